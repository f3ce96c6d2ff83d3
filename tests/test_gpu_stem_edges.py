"""The general stem kernels (csrc/stem_gen.hip: what every frame size other than 224 x 224 runs) element by element against float64 at
the shapes where their launch logic changes: tiles of 256 flattened pixels that hold the end of one frame and the start of the next,
the forward's grid-stride loop over at most 512 blocks, the weight gradient's over 512 blocks, the input gradient's M-tile tails and
col2im lane loop. Through the C ABI, every output pre-filled with NaN:

  r3m_stem_gen_prep          bit for bit torch CPU fp32 (x / 255 - mean) / std; bf16: that value rounded once
  r3m_stem_gen_fwd           with statistics and with stats = NULL: fp32 max-rel < 2e-5 of the range, bf16 max-rel < 2^-8 and l2-rel
                             < 2^-9 (util.assert_close_store); the BatchNorm partials per 256-pixel tile, 1e-4 of sum|y| and sum y^2
  r3m_stem_gen_wgrad         accumulate 0, then 1: max-rel < 5e-5 of the range against 1 x and 2 x the reference
  r3m_stem_gen_input_grad    accumulate 0, then 1 onto a non-zero base: max-rel < 2e-5 of the range, every element finite
  forward and input gradient frames 0, middle and last of an F-frame call bit-identical to 1-frame calls

The reference is float64 F.conv2d (+ autograd) on the operands the kernel multiplies: for bf16 the normalised image rounded once, the
bf16-rounded weights and the bf16 dY; the input gradient multiplies the (bf16) dZ with the fp32 master weights. The ceilings are the
ones the other operator tests use for the same stores (util.check_conv_fp32 / check_conv_bf16); none is fitted to these kernels. The
cases and the condition each is there for: util.STEM_EDGE_CASES, recomputed from (F, H, W) on the CPU by tests/test_stem_cases.py.
The bodies are in tests/util.py; one test per kernel, so that the largest case (35 x 126 x 125) stays at a few seconds each."""
import pytest

from util import (STEM_EDGE_CASES, check_stem_gen_forward, check_stem_gen_input_grad, check_stem_gen_prep, check_stem_gen_wgrad,
                  stem_case_id)

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("case", STEM_EDGE_CASES, ids=stem_case_id)
DTYPES = pytest.mark.parametrize("dtype", ["fp32", "bf16"])


@DTYPES
@CASES
def test_stem_gen_prep(hip, case, dtype):
    check_stem_gen_prep(hip, case, dtype)


@DTYPES
@CASES
def test_stem_gen_forward(hip, case, dtype):
    check_stem_gen_forward(hip, case, dtype)


@DTYPES
@CASES
def test_stem_gen_wgrad(hip, case, dtype):
    check_stem_gen_wgrad(hip, case, dtype)


@DTYPES
@CASES
def test_stem_gen_input_grad(hip, case, dtype):
    check_stem_gen_input_grad(hip, case, dtype)
