"""The linear self-attention launch (csrc/attn.hpp) on its own, through mpdx_attention_block - the code a network runs, on inputs a network never
produces: one tiny launch per case against the fp64 oracle (oracle.unet.linear_attention_block on the valid positions).  Shapes from the kernel's
own branch points, input regimes and the bound in tests/attn_ref.py; tests/test_oracle_attention_cpu.py shows that these cases tell wrong variants
of the block apart.

Measured on the MI355X, max|gpu - fp64| / e_ref (e_ref = max|fp32 CPU restatement - fp64|), the largest per regime over the shapes and batches:
plain 1.47, mean100 1.24, tinyvar 0.98, constrow 1.30, sharp64 1.65, sharp128 1.63, gsign 1.29, big 1.48 (table in DESIGN.md section 6);
K = 4 in attn_ref.py is twice the largest, rounded up.  The largest max|gpu - fp64| / bound is 0.38."""
import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ar.CASES, ids=[ar.case_id(c) for c in ar.CASES])
def test_block_vs_fp64_oracle(case):
    shape, regime = case
    C, L, Lv = shape
    problems = []
    single = {}   # trajectory b run alone (B = 1)
    for B in ar.SHAPES[shape]:
        bs = tuple(range(B))
        out = ar.run_block_gpu(shape, regime, bs)
        assert out.shape == (B, L, C)
        y = out[:, :Lv, :].transpose(1, 2)
        y64, e_ref, bound = ar.reference(shape, regime, bs)
        err = float((y.double() - y64).abs().max())
        print(f"{ar.case_id(case)} B={B}: max|gpu-fp64| = {err:.3e}  e_ref = {e_ref:.3e}  ratio = {err / e_ref:.2f}  bound = {bound:.3e}  max|y| = {float(y64.abs().max()):.3e}")
        if not bool(torch.isfinite(out).all()):
            problems.append((B, "not finite"))
        if int(torch.count_nonzero(out[:, Lv:, :])):
            problems.append((B, "pad rows are not zero"))
        if not err <= bound:
            problems.append((B, f"max|gpu-fp64| = {err:.3e} > {bound:.3e}"))
        for b in sorted({0, B // 2, B - 1}):   # a trajectory's rows do not depend on the batch, nor on its place in the workgroup
            if b not in single:
                single[b] = out[0] if B == 1 else ar.run_block_gpu(shape, regime, (b,))[0]
            if not torch.equal(single[b], out[b]):
                problems.append((B, f"trajectory {b} differs from its B = 1 run by {float((single[b] - out[b]).abs().max()):.3e}"))
    assert not problems, problems


@pytest.mark.parametrize("shape", ar.REFUSED, ids=[f"C{c}_L{l}" for c, l, _ in ar.REFUSED])
def test_block_refusals_launch_nothing(shape):
    C, L, Lv = shape
    x = torch.ones((2, L, C), device="cuda")
    with pytest.raises(RuntimeError, match="self-attention block"):
        ar.run_block_gpu_raw(x, ar.block_params(32, "plain"), L, Lv, C)
    torch.cuda.synchronize()
    assert bool((x == 1).all())
