"""row_moments (csrc/recall_epilogue.hip): per-row mean and correction=1
standard deviation of a bf16 matrix in one pass, against numpy fp64 over the
same bf16 values.

Tolerances, from the kernel's arithmetic and not from its output: the sums
are fp64 and shifted by the row's first element, so
  |mu - mu64|  <= 2^-23 |mu64| + m 2^-52 max|s|   (one fp32 rounding of the
                  result plus the fp64 summation bound),
  |sigma - sigma64| <= 2^-22 sigma64, or 2^-22 max|s| absolute where sigma64
                  is 0;
the shifted form has no cancellation term to add."""

import numpy as np
import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rows(nq, m, seed):
    """bf16 [nq, m]: row 0 random, then (nq = 5) the clustered case (mean
    about 0.5, std about 0.01), a constant row, a wide row and a row whose
    first element is far from the rest."""
    gen = torch.Generator().manual_seed(seed)
    S = torch.randn(nq, m, generator=gen) * 0.05
    if nq >= 5:
        S[1] = 0.5 + 0.01 * torch.randn(m, generator=gen)
        S[2] = 0.337
        S[3] = torch.randn(m, generator=gen) * 3.0 - 1.0
        S[4] = -0.25 + 0.02 * torch.randn(m, generator=gen)
        S[4, 0] = 0.75
    return S.bfloat16()


def _check(S):
    nq, m = S.shape
    x = S.float().numpy().astype(np.float64)  # the bf16 values, exactly
    # reference sums over x - x[0], an exact fp64 subtraction: the same
    # numbers, and a constant row then has a standard deviation of exactly 0
    # instead of the rounding residue of its own mean
    x0 = x[:, :1]
    mu64 = x0[:, 0] + (x - x0).mean(axis=1)
    sg64 = (x - x0).std(axis=1, ddof=1)
    smax = np.abs(x).max(axis=1)
    Sg = S.to(DEV)
    mu, sigma = g.row_moments(Sg)
    mu2, sigma2 = g.row_moments(Sg)
    assert mu.dtype == torch.float32 and sigma.dtype == torch.float32
    assert mu.shape == (nq,) and sigma.shape == (nq,) and mu.is_cuda
    assert torch.equal(mu, mu2) and torch.equal(sigma, sigma2)  # fixed order
    mu = mu.cpu().numpy().astype(np.float64)
    sigma = sigma.cpu().numpy().astype(np.float64)
    mu_err = np.abs(mu - mu64)
    mu_tol = 2.0 ** -23 * np.abs(mu64) + m * 2.0 ** -52 * smax
    sg_err = np.abs(sigma - sg64)
    sg_tol = np.where(sg64 > 0, 2.0 ** -22 * sg64, 2.0 ** -22 * smax)
    print(f"nq={nq} m={m} mu err/tol {np.max(mu_err / mu_tol):.3f} "
          f"sigma err/tol {np.max(sg_err / sg_tol):.3f}")
    assert (mu_err <= mu_tol).all(), (mu_err, mu_tol)
    assert (sg_err <= sg_tol).all(), (sg_err, sg_tol)
    return mu64, sg64, sigma


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("m", [2, 3, 7, 8, 9, 1000])
def test_row_moments_small(m, nq):
    S = _rows(nq, m, seed=100 + m)
    mu64, sg64, sigma = _check(S)
    if nq == 5:
        assert sg64[2] == 0.0 and sigma[2] == 0.0  # the constant row
        if m == 1000:
            assert abs(mu64[1] - 0.5) < 0.01 and 0.005 < sg64[1] < 0.02


@pytest.mark.parametrize("clustered", [False, True])
def test_row_moments_sample_width(clustered):
    # the width of the threshold pre-pass sample, one row
    m = 131072
    gen = torch.Generator().manual_seed(9)
    S = torch.randn(1, m, generator=gen) * 0.03
    if clustered:
        S = 0.5 + S / 3.0
    _check(S.bfloat16())


def test_row_moments_matmul_output():
    # what topk_recall_threshold passes: the matmul's own output
    torch.manual_seed(3)
    Q = torch.nn.functional.normalize(torch.randn(5, 64), dim=1).bfloat16().to(DEV)
    X = torch.nn.functional.normalize(torch.randn(333, 64), dim=1).bfloat16().to(DEV)
    S = torch.matmul(Q, X.T)
    assert S.dtype == torch.bfloat16 and S.is_contiguous()
    _check(S.cpu())
