"""The comparison rules of the float64 kernel tests, one definition for
tests/test_small_kernels_f64_gpu.py and tests/test_gemm_conv_f64_gpu.py.

With ref64 the plain float64 definition (tests/f64_reference.py) and torch32
torch's own fp32 implementation on the GPU, fed the same inputs,

    e_torch  = max |torch32 - ref64|        e_kernel = max |kernel - ref64|

cmp() asserts  e_kernel <= 4 * e_torch + 4 * eps32 * max|ref64|  (factor 4: a
different but equally valid summation order; the ulp floor covers ops where
torch is exact), and that NaN and inf sit exactly where the reference has
them.  Each comparison prints one `F64 | family | what | ...` line, from which
the modules' docstring tables are made.
"""

import torch

EPS32 = 2.0 ** -23


def cpu64(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


def cmp(family, what, kernel, torch32, ref64):
    """the tolerance rule; NaN and inf placement must equal the reference's"""
    k, t, r = cpu64(kernel), cpu64(torch32), cpu64(ref64)
    assert k.shape == r.shape == t.shape, f"{family} {what}: shapes"
    nan, inf = torch.isnan(r), torch.isinf(r)
    assert torch.equal(torch.isnan(k), nan), f"{family} {what}: NaN placement"
    assert torch.equal(k[inf], r[inf]), f"{family} {what}: inf placement"
    fin = ~(nan | inf)
    if not bool(fin.any()):
        return
    e_kernel = float((k[fin] - r[fin]).abs().max())
    e_torch = float((t[fin] - r[fin]).abs().max())
    bound = 4.0 * e_torch + 4.0 * EPS32 * float(r[fin].abs().max())
    print(f"F64 | {family} | {what} | e_kernel {e_kernel:.3e} | "
          f"e_torch {e_torch:.3e} | bound {bound:.3e}")
    assert e_kernel <= bound, (
        f"{family} {what}: e_kernel {e_kernel:.3e} > bound {bound:.3e} "
        f"(e_torch {e_torch:.3e})")


def exact(ours, theirs, what):
    """exact equality; NaN equals NaN"""
    a, b = ours.detach().cpu(), theirs.detach().cpu()
    assert a.shape == b.shape, what
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN placement"
    ok = (a == b) | torch.isnan(b)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {a.numel()} differ"
