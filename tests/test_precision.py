"""CPU proof that the bounds of tests/precision.py tell a correct bf16x3 product from a subtly wrong one.

For every GEMM case of precision.CASES (true K and k chain, fewer rows and columns), the emulated six-term product must
stay well below its bound and, for chains of at most 256, every variant that lost a 2^-16 term, or all three of them,
well above it; on uniform and on mixed-scale inputs (longer chains: precision.X3_TIERS).  The printed table (pytest -s)
is the evidence the bounds were chosen from.
"""
import pytest
import torch

from tests import precision as P


def _inputs(M, K, N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(M, K, generator=g) * 2 - 1
    B = torch.rand(K, N, generator=g) * 2 - 1
    if kind == "mixed":
        B = B * P.mixed_scales("in", K, *P.IN_SCALES)[:, None]
        A = A * P.mixed_scales("row", M, *P.ROW_SCALES)[:, None]
    return A, B


def _tier(chain):
    for top, bound, six_frac, wrong_mult in P.X3_TIERS:
        if chain <= top:
            return bound, six_frac, wrong_mult
    raise AssertionError(chain)


@pytest.mark.parametrize("case", P.CASES, ids=[c["name"] for c in P.CASES])
def test_bound_separates_the_six_term_product_from_a_lost_term(case):
    K, chain = case["K"], case["chain"]
    bound, six_frac, wrong_mult = _tier(chain)
    assert P.case_bound(case) == bound
    M = min(case["M"], 32)
    N = 16 if K > 20000 else max(128, 2048 // M)       # (few rows: more columns, for a stable maximum)
    slice_len = None if chain >= K else -(-chain // 16) * 16
    rows = []
    for kind in ("uniform", "mixed"):
        A, B = _inputs(M, K, N, kind, seed=K)
        ref = A.double() @ B.double()
        six = P.rel_err_rows(P.emulate_x3(A, B, P.SIX, slice_len=slice_len), ref, (0,))
        wrong = {k: P.rel_err_rows(P.emulate_x3(A, B, t, slice_len=slice_len), ref, (0,)) for k, t in P.WRONG.items()}
        rows.append((kind, six, wrong))
        print("%-26s %-7s chain %6d bound %.2e | six %.2e | %s" % (case["name"], kind, chain, bound, six,
                                                                   " ".join("%s %.2e" % kv for kv in wrong.items())))
    for kind, six, wrong in rows:
        assert six <= six_frac * bound, (kind, six, bound)
        for k, e in wrong.items():
            assert wrong_mult is None or e >= wrong_mult * bound, (kind, k, e, bound)


def test_split_is_exact_and_rounds_to_nearest_even():
    x = torch.tensor([1 + 2 ** -8, 1 + 2 ** -8 + 2 ** -16, -(1 + 2 ** -8), -(1 + 2 ** -8 + 2 ** -16), 3.0e-3, -7.5],
                     dtype=torch.float32)
    h, m, lo = P.split3(x)
    assert torch.equal(h + m + lo, x.double())
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7: even mantissa -> 1, remainder +2^-8
    assert h[0] == 1 and m[0] == 2 ** -8 and lo[0] == 0
    # 1 + 2^-8 + 2^-16 lies above the tie: rounds up, the mid piece changes sign
    assert h[1] == 1 + 2 ** -7 and m[1] == -(2 ** -8 - 2 ** -16) and lo[1] == 0
    assert h[2] == -1 and m[2] == -(2 ** -8)
    assert h[3] == -(1 + 2 ** -7) and m[3] == 2 ** -8 - 2 ** -16


def test_emulated_split_k_adds_the_slices_in_order():
    A, B = _inputs(8, 640, 16, "uniform", 3)
    whole = P.emulate_x3(A, B)
    sliced = P.emulate_x3(A, B, slice_len=128)
    ref = A.double() @ B.double()
    assert P.rel_err_rows(whole, ref, (0,)) <= P.X3_BOUND and P.rel_err_rows(sliced, ref, (0,)) <= P.X3_BOUND
    parts = [P.emulate_x3(A[:, i:i + 128], B[i:i + 128]) for i in range(0, 640, 128)]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    assert torch.equal(sliced, acc)


def test_row_metric_sees_an_error_in_a_small_row():
    """A 1e-3 relative error in a row of magnitude 1e-3 beside rows of magnitude 1: the suite's `close()` (absolute
    error <= rtol * max(1, max|ref|)) accepts it, the row-normalised metric does not."""
    g = torch.Generator().manual_seed(5)
    ref = (torch.rand(2, 4, 8, 8, generator=g, dtype=torch.float64) * 2 - 1)
    ref[1, 2] *= 1e-3
    got = ref.clone()
    got[1, 2] *= 1 + 1e-3
    got = got.float()
    scale = max(1.0, float(ref.abs().max()))
    assert float((got.double() - ref).abs().max()) <= 2e-5 * scale       # what close(..., rtol=2e-5) lets through
    assert P.rel_err_rows(got, ref, (0, 1)) >= 0.9e-3
    assert P.rel_err_rows(ref.float(), ref, (0, 1)) <= 2 ** -24


def test_row_metric_zero_rows():
    ref = torch.zeros(2, 3, 4, dtype=torch.float64)
    ref[0, 1] = 1.0
    assert P.rel_err_rows(ref.clone(), ref, (0, 1)) == 0.0
    bad = ref.clone()
    bad[1, 2, 3] = 1e-30
    assert P.rel_err_rows(bad, ref, (0, 1)) == float("inf")
    assert P.rel_err_rows(ref.t() if ref.dim() == 2 else ref[0], ref[0], (0,)) == 0.0


def test_mixed_scales_span_their_range():
    s = P.mixed_scales("in", 96, *P.IN_SCALES)
    assert float(s.min()) == 2.0 ** -10 and float(s.max()) == 2.0 ** 10
    assert torch.equal(torch.log2(s), torch.round(torch.log2(s)))
