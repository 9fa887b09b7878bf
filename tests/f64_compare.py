"""The comparison rules of the float64 kernel tests, one definition for
tests/test_small_kernels_f64_gpu.py, tests/test_gemm_conv_f64_gpu.py and
tests/test_wino_f64_gpu.py.

With ref64 the plain float64 definition (tests/f64_reference.py) and torch32
torch's own fp32 implementation on the GPU, fed the same inputs,

    e_torch  = max |torch32 - ref64|        e_kernel = max |kernel - ref64|

cmp() asserts  e_kernel <= 4 * e_torch + 4 * eps32 * max|ref64|  (factor 4: a
different but equally valid summation order; the ulp floor covers ops where
torch is exact), and that NaN and inf sit exactly where the reference has
them.  Each comparison prints one `F64 | family | what | ...` line, from which
the modules' docstring tables are made.

The yardstick need not be torch's op: where torch runs another algorithm than
the kernel (its direct conv against a Winograd kernel), the rule is applied
with a plain fp32 implementation of the kernel's own algorithm in torch32's
place (`yard` names it in the line), and torch's error goes into the line
through `also`, for the table, asserting nothing.

_ceiling() needs no yardstick: |kernel - ref| <= (terms + 1) * 2^-23 * abs64 for
every element, abs64 the op over the magnitudes of its operands in double: the
bound of an fp32 chain of `terms` roundings in any order.
"""

import torch

EPS32 = 2.0 ** -23


def cpu64(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


def cmp(family, what, kernel, torch32, ref64, yard="torch", also=None):
    """the tolerance rule; NaN and inf placement must equal the reference's.
    also: {name: tensor} whose errors are printed only"""
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
    more = "".join(f" | e_{name} {float((cpu64(v)[fin] - r[fin]).abs().max()):.3e}"
                   for name, v in (also or {}).items())
    print(f"F64 | {family} | {what} | e_kernel {e_kernel:.3e} | "
          f"e_{yard} {e_torch:.3e}{more} | bound {bound:.3e}")
    assert e_kernel <= bound, (
        f"{family} {what}: e_kernel {e_kernel:.3e} > bound {bound:.3e} "
        f"(e_{yard} {e_torch:.3e})")


def exact(ours, theirs, what):
    """exact equality; NaN equals NaN"""
    a, b = ours.detach().cpu(), theirs.detach().cpu()
    assert a.shape == b.shape, what
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN placement"
    ok = (a == b) | torch.isnan(b)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {a.numel()} differ"


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _draw(kind, shape, g):
    """exact: integers from [-4, 4]; randn: standard normal"""
    if kind == "exact":
        return torch.randint(-4, 5, shape, generator=g).float()
    return torch.randn(shape, generator=g)


def _ceiling(family, what, kernel, ref64, abs64, terms):
    """|kernel - ref| <= (terms + 1) * 2^-23 * sum |a||b|, element by element"""
    k, r, lim = cpu64(kernel), cpu64(ref64), (terms + 1) * EPS32 * cpu64(abs64)
    fin = torch.isfinite(r)
    err = (k - r).abs()[fin]
    lim = lim[fin]
    pos = lim > 0
    share = float((err[pos] / lim[pos]).max()) if bool(pos.any()) else 0.0
    print(f"CEIL | {family} | {what} | terms {terms} | share {share:.3e}")
    assert bool((err <= lim).all()), (
        f"{family} {what}: {int((err > lim).sum())} elements past the fma-chain "
        f"ceiling, worst share {share:.3e}")
