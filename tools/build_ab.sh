#!/bin/bash
# A/B builds for same-box comparisons (gitignored *.so):
#   r3m_amd/lib/libr3m_hip_base.so   = csrc/ of a git ref (default HEAD)             -> R3M_HIP_LIB=... python bench.py
#   r3m_amd/lib/libr3m_hip_probes.so = the working tree with -DR3M_PROBES (environment switches live)
#   r3m_amd/lib/libr3m_hip_<name>.so = the working tree with extra compiler flags (compile-time experiment switches)
# usage: tools/build_ab.sh [base-ref|none] [probes | variant <name> <flags...>]
set -e
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
REF="${1:-HEAD}"
build_tree() {   # $1 = source root holding r3m_amd/csrc + include, $2 = output .so, $3.. = extra flags (one source list: csrc/build.sh)
  local src="$1" out="$2"; shift 2
  R3M_BUILD_SRC="$src" R3M_BUILD_OUT="$out" bash "$ROOT/r3m_amd/csrc/build.sh" "$@"
}
if [ "$REF" != "none" ]; then
  T="$(mktemp -d)"; (cd "$ROOT" && git archive "$REF" r3m_amd/csrc include | tar -x -C "$T")
  build_tree "$T" "$ROOT/r3m_amd/lib/libr3m_hip_base.so"; rm -rf "$T"
fi
if [ "$2" = "probes" ]; then build_tree "$ROOT" "$ROOT/r3m_amd/lib/libr3m_hip_probes.so" -DR3M_PROBES; fi
if [ "$2" = "variant" ]; then N="$3"; shift 3; build_tree "$ROOT" "$ROOT/r3m_amd/lib/libr3m_hip_$N.so" "$@"; fi
