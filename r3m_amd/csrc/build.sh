#!/bin/bash
# Builds libr3m_hip.so for gfx950 (MI355X). hipcc cross-compiles without a GPU. Usage: build.sh [extra hipcc flags]
# A/B builds (tools/build_ab.sh): R3M_BUILD_SRC = root of another source tree (holding r3m_amd/csrc and include), R3M_BUILD_OUT = the
# .so to write; with R3M_BUILD_OUT set every source is compiled afresh into a temporary directory (the flags may differ).
set -e
ROOT="${R3M_BUILD_SRC:-$(cd "$(dirname "${BASH_SOURCE[0]}")/../.." && pwd)}"
HERE="$ROOT/r3m_amd/csrc"
LIB="${R3M_BUILD_OUT:-$ROOT/r3m_amd/lib/libr3m_hip.so}"
if [ -n "$R3M_BUILD_OUT" ]; then OBJ="$(mktemp -d)"; trap 'rm -rf "$OBJ"' EXIT; else OBJ="$ROOT/build/obj"; fi
mkdir -p "$(dirname "$LIB")" "$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $*"
# at most MAX_JOBS (default: the CPU count, at most 16) compiles at once; a failed compile is named on stdout and stderr
JOBS="${MAX_JOBS:-$(nproc 2>/dev/null || echo 8)}"
[ "$JOBS" -ge 1 ] 2>/dev/null || JOBS=8
[ "$JOBS" -gt 16 ] && JOBS=16
launched=""
SRCS="conv conv_pw conv_small wgrad wgrad_win conv_bf16 wgrad_bf16 conv_row16 conv_pw16 stem stem_bf16 stem_dgrad stem_gen bn bn_pool feat loss adam lang text augment engine capi"
for f in $SRCS; do
  [ -f "$HERE/$f.hip" ] || continue
  stale=0
  [ -f "$OBJ/$f.o" ] || stale=1
  for dep in "$HERE/$f.hip" "$HERE"/*.h "$ROOT/include/r3m_hip.h" "$HERE/build.sh"; do
    [ "$dep" -nt "$OBJ/$f.o" ] && stale=1
  done
  if [ $stale = 1 ]; then
    EXTRA=""
    # conv_pw16: the tile tickets are requested one tile before they are used; the wave-level atomic optimizer would wait for each at once
    [ "$f" = conv_pw16 ] && EXTRA="-mllvm -amdgpu-atomic-optimizer-strategy=None"
    while [ "$(jobs -rp | wc -l)" -ge "$JOBS" ]; do wait -n || true; done
    rm -f "$OBJ/$f.rc" "$OBJ/$f.o"
    launched="$launched $f"
    ( rc=0; $HIPCC $FLAGS $EXTRA -c "$HERE/$f.hip" -o "$OBJ/$f.o" || rc=$?; echo "$rc" > "$OBJ/$f.rc" ) &
  fi
done
wait
failed=""
for f in $launched; do
  rc="$(cat "$OBJ/$f.rc" 2>/dev/null || echo killed)"
  rm -f "$OBJ/$f.rc"
  if [ "$rc" != 0 ]; then failed="$failed $f.hip($rc)"; rm -f "$OBJ/$f.o"; fi
done
if [ -n "$failed" ]; then
  echo "build.sh: compile failed:$failed"
  echo "build.sh: compile failed:$failed" >&2
  exit 1
fi
objs=()
for f in $SRCS; do [ -f "$OBJ/$f.o" ] && objs+=("$OBJ/$f.o"); done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$LIB" "${objs[@]}"
echo "built $LIB"
