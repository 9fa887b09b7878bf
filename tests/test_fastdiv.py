"""FastDiv (ops/csrc/common.h): q = (n * m) >> 40 with m = 2^40 // d + 1.

The kernels decode every tensor index with it.  It is exact only while
n * d < 2^40 (and n * m fits 64 bits); past that a quotient is one too large
and the remainder wraps as unsigned.  fast_div() (torch_util.h), the only way
to fill one, is given the largest dividend the kernel forms and refuses the
pair otherwise.  These tests run the host build of div() through the bound
evaluator; they launch nothing and need no GPU.
"""

import numpy as np
import pytest

LIMIT = 1 << 40


def _native():
    from split_learning_amd.ops import native
    return native()


def _magic(d):
    return LIMIT // d + 1


def _max_n(d):
    """the largest dividend the checked initialiser admits for d"""
    return min((1 << 31) - 1, (LIMIT - 1) // d, ((1 << 64) - 1) // _magic(d))


DIVISORS = [1, 2, 3, 5, 7, 11, 13, 97, 127, 251, 257, 509, 521, 4093, 65521,
            2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, 262144, 524176, 2 ** 20 - 1, 2 ** 20,
            2 ** 20 + 1, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 32 - 1]


@pytest.mark.parametrize("d", DIVISORS)
def test_div_is_exact_up_to_the_checked_limit(d):
    max_n = _max_n(d)
    qmax = max_n // d
    rng = np.random.default_rng(d)
    qs = {0, 1, 2, 3, qmax // 2, qmax - 1, qmax}
    qs.update(int(q) for q in rng.integers(0, qmax + 1, size=2000))
    ns = {max_n, max_n - 1}
    for q in qs:
        ns.update((q * d - 1, q * d, q * d + d - 1))
    ns = sorted(n for n in ns if 0 <= n <= max_n)
    got = _native().fast_div_eval(d, max_n, ns)
    bad = [(n, g) for n, g in zip(ns, got) if g != n // d]
    assert not bad, f"d={d}: (n, div(n)) {bad[:5]} of {len(bad)} wrong"


@pytest.mark.parametrize("d", DIVISORS)
def test_one_past_the_limit_is_refused(d):
    with pytest.raises(RuntimeError, match="fast_div_eval.*FastDiv"):
        _native().fast_div_eval(d, _max_n(d) + 1, [])


def test_zero_divisor_divides_as_one():
    assert _native().fast_div_eval(0, 5, [0, 3, 5]) == [0, 3, 5]


# divisor, the first dividend whose unchecked quotient is wrong, a shape that
# reaches it
FIRST_WRONG = [
    (262144, 4456447),    # conv, batch 17, 512x512 output
    (524176, 2620879),    # 724x724 output, batch 5
    (1048576, 2097151),   # BatchNorm on (1, 3, 1024, 1024), maxpool on (1, 2, 2048, 2048)
    (1048577, 1048576),   # a single 1025x1023 image
    (1, 1 << 24),         # n * m leaves 64 bits
]


@pytest.mark.parametrize("d,first", FIRST_WRONG)
def test_unchecked_arithmetic_goes_wrong_where_the_guard_says(d, first):
    """the same multiply and shift in numpy uint64 (wrapping as the hardware
    does): right below `first`, wrong at it, and the guard's limit lies below
    it"""
    n = np.arange(first + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        q = (n * np.uint64(_magic(d))) >> np.uint64(40)
    wrong = np.nonzero(q != n // np.uint64(d))[0]
    assert wrong.tolist() == [first]
    assert _max_n(d) < first
