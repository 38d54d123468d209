"""The measuring stick of the bf16x3 precision tests (tests/test_precision.py on the CPU, tests/test_precision_gpu.py on
the device).

Every matrix-core contraction of the project splits its fp32 operands three ways, x = h + m + l with h = bf16(x),
m = bf16(x - h), l = bf16(x - h - m) (round to nearest even, pir_split8 in gemm_common.h), and runs the six products
above 2^-24 as bf16 MFMAs with fp32 accumulation: per 16-deep k-step the terms l*h, h*l, m*m, m*h, h*m, h*h, in that
order, into one accumulator; split-K slices are added in order by a second stage.  `emulate_x3` restates that on the
CPU, with any subset of the terms, so the CPU test can show that `X3_BOUND` lies above the error of the six-term product
and well below the error of a product that lost one of its 2^-16 terms.

The error is normalised per output row (`rel_err_rows`): one output channel of one image, so rows of small magnitude
(row-scale epilogues, LayerNorm on load, mixed-scale weights) are judged on their own scale.
"""
from __future__ import annotations

from typing import Iterable, Sequence, Tuple

import numpy as np
import torch

# (piece of A, piece of B): 0 = hi, 1 = mid, 2 = lo; in the kernels' per-accumulator order (pir_mfma_x3)
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
DROP_MM = tuple(t for t in SIX if t != (1, 1))      # one 2^-16 term dropped: mid x mid
DROP_LH = tuple(t for t in SIX if t != (2, 0))      # ... lo x hi (the weight's lo piece lost)
DROP_HL = tuple(t for t in SIX if t != (0, 2))      # ... hi x lo (the activation's lo piece lost)
THREE = ((1, 0), (0, 1), (0, 0))                    # "bf16x2": hi x hi, mid x hi, hi x mid
WRONG = {"drop_mm": DROP_MM, "drop_lh": DROP_LH, "drop_hl": DROP_HL, "three": THREE}

# Bound on the row-normalised error (vs float64) of one bf16x3 product whose accumulator runs a k chain of at most 256
# (the 1x1 convolutions with 48 .. 192 input channels, the first dense 3x3 convolution).  Chosen by tests/test_precision.py:
# the emulated six-term product stays below 0.6 x the bound, every variant that lost a 2^-16 term lies above 2 x the
# bound (the table the test prints).
X3_BOUND = 1.0e-6
# Longer chains: each of the six MFMAs of a k-step rounds the fp32 accumulator, so the six-term error grows with the chain
# (emulation, both input kinds: 2-3e-7 at k <= 192, 4.5-8.3e-7 at 384 .. 510, up to 9.6e-7 at 1152, 1.9e-6 at 2880 ..
# 4096) while the error of a dropped 2^-16 term does not (2.1e-6 .. 6e-6 at every length).  Past k = 256 the two cannot
# be told apart: on the device (many more rows and columns than the emulation, so larger maxima) the correct kernels
# measured 1.76e-6 at k = 510 and 3.09e-6 at k = 3456.  These tiers bound the accumulation error only; a lost term is
# caught by the chains of at most 256 every 1x1 family also runs (tests/test_precision_gpu.py asserts each family ran
# one: K = 48 .. 192, or K cut by the split over k), the dense 3x3 kernels at K = 27, the split-K weight gradients and
# the one-hot / identity exactness tests.
#   (longest chain, bound, six-term error at most this fraction of it, dropped-term error at least this multiple or None)
X3_TIERS = ((256, X3_BOUND, 0.6, 2.0), (1152, 2.2e-6, 0.5, None), (6912, 4.5e-6, 0.6, None))


def x3_bound(chain: int) -> float:
    """The bound for a bf16x3 product whose longest fp32 accumulation chain is `chain` k values."""
    for top, bound, _, _ in X3_TIERS:
        if chain <= top:
            return bound
    raise ValueError("no bound recorded for a k chain of %d" % chain)


def split3(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 -> (hi, mid, lo) as float64 tensors holding bf16 values (round to nearest even, like pir_split8)."""
    x = x.float()
    h = x.to(torch.bfloat16).float()
    r1 = x - h
    m = r1.to(torch.bfloat16).float()
    r2 = r1 - m
    lo = r2.to(torch.bfloat16).float()
    return h.double(), m.double(), lo.double()


def emulate_x3(A: torch.Tensor, B: torch.Tensor, terms: Sequence[Tuple[int, int]] = SIX, kstep: int = 16,
               slice_len: int = None) -> torch.Tensor:
    """C = A B ([M, K] x [K, N]) as the kernels compute it: the terms of the split product per k-step of `kstep`, each
    added to an fp32 accumulator (the 16 bf16 products of one MFMA k-step summed exactly, one rounding); the k range cut
    into slices of `slice_len` (a multiple of kstep; None: one chain) whose fp32 sums are added in order."""
    M, K = A.shape
    N = B.shape[1]
    kp = -(-K // kstep) * kstep
    slice_len = kp if slice_len is None else slice_len
    assert slice_len % kstep == 0
    ns = -(-kp // slice_len)
    kpad = ns * slice_len
    Ap = torch.zeros(M, kpad, dtype=torch.float32)
    Bp = torch.zeros(kpad, N, dtype=torch.float32)
    Ap[:, :K], Bp[:K] = A.float(), B.float()
    pa, pb = split3(Ap), split3(Bp)
    steps = slice_len // kstep
    # [slice, step, kstep, ...]
    pa = [p.reshape(M, ns, steps, kstep).permute(1, 2, 0, 3) for p in pa]          # [ns, steps, M, kstep]
    pb = [p.reshape(ns, steps, kstep, N) for p in pb]                              # [ns, steps, kstep, N]
    prods = {t: torch.matmul(pa[t[0]], pb[t[1]]) for t in set(terms)}            # float64 [ns, steps, M, N]
    acc = torch.zeros(ns, M, N, dtype=torch.float32)
    for s in range(steps):
        for t in terms:
            acc = (acc.double() + prods[t][:, s]).float()
    out = acc[0]
    for s in range(1, ns):
        out = out + acc[s]
    return out


def rel_err_rows(got: torch.Tensor, ref64: torch.Tensor, row_dims: Iterable[int] = (0, 1)) -> float:
    """max over output rows of max|got - ref| / max|ref|; a row is one index of `row_dims` (one output channel of one image
    for (0, 1) on [B, C, H, W]; (0,) for a [rows, cols] matrix).  A row whose reference is all zero counts 0 when `got` is
    exactly zero there too, and infinity otherwise."""
    got = got.detach().cpu().double()
    ref = ref64.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rd = sorted(int(d) % ref.dim() for d in row_dims)
    rest = [d for d in range(ref.dim()) if d not in rd]
    nrows = int(np.prod([ref.shape[d] for d in rd])) if rd else 1
    g = got.permute(*rd, *rest).reshape(nrows, -1)
    r = ref.permute(*rd, *rest).reshape(nrows, -1)
    diff = (g - r).abs().amax(dim=1)
    scale = r.abs().amax(dim=1)
    err = torch.where(diff == 0, torch.zeros_like(diff), diff / scale)     # 0/0 -> 0, x/0 -> inf
    return float(err.max())


def mixed_scales(name: str, n: int, lo: float, hi: float) -> torch.Tensor:
    """n power-of-two scales 2^e, e uniform over [lo, hi] (deterministic per name); both ends included."""
    from promptir_amd import weights as W

    u = W.uniform01(name + "#scale", n, 0).astype(np.float64)
    e = np.round(lo + (hi - lo) * u)
    if n >= 2:
        e[0], e[-1] = lo, hi
    return torch.from_numpy(np.exp2(e).astype(np.float32))


# Mixed-scale inputs: activations scaled per input channel over 2^-10 .. 2^10, weights per output row over 2^-12 .. 1.
IN_SCALES = (-10, 10)
ROW_SCALES = (-12, 0)


# The GEMM shapes of the model the GPU test drives through every family, and their k chains: M = output rows, K = the
# contraction, chain = the longest k range one accumulator runs without a split (a split over k, knobs 44 / 45, only
# shortens it).  1x1 forward / input gradient: K = input channels; dense 3x3: K = 9 x input channels; weight gradients:
# K = batch x pixels, cut by the split-K gemm_nt into slices of at least 128 pixels (the emulation takes 4096).
CASES = [
    dict(name="1x1 48->144 @128", M=144, K=48, chain=48, family="1x1"),
    dict(name="1x1 96->510 @128", M=510, K=96, chain=96, family="1x1"),
    dict(name="1x1 510->96 @128", M=96, K=510, chain=510, family="1x1"),
    dict(name="1x1 192->1020 @32", M=1020, K=192, chain=192, family="1x1"),
    dict(name="1x1 384->2042 @16", M=2042, K=384, chain=384, family="1x1"),
    dict(name="1x1 2042->384 @16", M=384, K=2042, chain=2042, family="1x1 (knob 45 splits)"),
    dict(name="3x3 3->48 @128", M=48, K=27, chain=27, family="3x3"),
    dict(name="3x3 48->24 @128", M=24, K=432, chain=432, family="3x3"),
    dict(name="3x3 96->3 @128", M=3, K=864, chain=864, family="3x3"),
    dict(name="3x3 96->192 @64", M=192, K=864, chain=864, family="3x3"),
    dict(name="3x3 64->64 @64 prompt", M=64, K=576, chain=576, family="3x3"),
    dict(name="3x3 128->128 @32 prompt", M=128, K=1152, chain=1152, family="3x3 (knob 44 splits)"),
    dict(name="3x3 192->384 @32", M=384, K=1728, chain=1728, family="3x3 (knob 44 splits)"),
    dict(name="3x3 320->320 @16 prompt", M=320, K=2880, chain=2880, family="3x3 (knob 44 splits)"),
    dict(name="3x3 384->768 @16", M=768, K=3456, chain=3456, family="3x3 (knob 44 splits)"),
    dict(name="3x3 dgrad 768->384 @16", M=384, K=6912, chain=6912, family="3x3 (knob 44 splits)"),
    dict(name="wgrad 1x1 b8 @16", M=384, K=8 * 256, chain=2048, family="gemm_nt"),
    dict(name="wgrad 1x1 b8 @128", M=144, K=8 * 16384, chain=4096, family="gemm_nt split-K"),
    dict(name="mdta gram hw 16384", M=48, K=16384, chain=4096, family="gemm_nt split-K"),
]


def case_bound(case) -> float:
    return x3_bound(case["chain"])
