"""fp4_mx_spec (the integer-only statement of the quantize kernel's
contract) against to_fp4_mx (the oracle), bit for bit, on the CPU."""

import pytest
import torch

from vainplex_openclaw_amd.ops import gpu as g


def crafted_rows(D: int = 128) -> torch.Tensor:
    """The hand-made rows the quantize tests share (bf16 [r, D], D % 128
    == 0): zero row, single non-zero, every e2m1 midpoint with both signs
    under a 6.0 max (the tie cases), a small negative next to 6.0 (the
    negative-zero code), group maxima 1.5 * 2^j, subnormals."""
    rows = []
    rows.append(torch.zeros(D))
    one = torch.zeros(D)
    one[37] = -0.3125
    rows.append(one)
    mids = torch.tensor(g._E2M1_MIDPOINTS)
    ties = torch.zeros(D)
    # every 32-element scale group of the first chunk gets max 6.0 and all
    # fourteen signed midpoints; element -> group follows fp4_perm128
    perm = g.fp4_perm128()
    for grp in range(4):
        el = perm[grp * 32:(grp + 1) * 32]
        ties[el[0]] = 6.0
        ties[el[1:8]] = mids
        ties[el[8:15]] = -mids
        ties[el[16]] = -6.0
        ties[el[17:24]] = mids * 0.5   # exact halves: below / on lower midpoints
    rows.append(ties)
    negz = torch.zeros(D)
    negz[0::2] = -0.01
    negz[1] = 6.0
    negz[65] = -6.0
    rows.append(negz)
    for j in (-130, -126, -20, -1, 0, 1, 7, 100, 126):
        r = torch.full((D,), 2.0 ** max(j - 3, -133))
        r[5] = 1.5 * 2.0 ** j
        r[70] = -1.25 * 2.0 ** j       # a max just below the 1.5 boundary
        r[90] = 1.5078125 * 2.0 ** j   # the first bf16 above it
        rows.append(r)
    sub = torch.zeros(D)
    sub[0::3] = 2.0 ** -133            # bf16 subnormals
    sub[1::3] = -3 * 2.0 ** -130
    sub[2] = 2.0 ** -127
    rows.append(sub)
    mixed = torch.randn(D, generator=torch.Generator().manual_seed(3))
    mixed[::7] *= 2.0 ** -120          # tiny values under a normal max
    rows.append(mixed)
    return torch.stack(rows).bfloat16()


def all_finite_bf16_as_maxima() -> torch.Tensor:
    """One 32-element scale group per finite bf16 bit pattern, which is the
    group's max |v|; the rest of the group are fractions of it."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]                     # drop inf/nan
    vmax = bits.to(torch.int16).view(torch.bfloat16).float()   # [65280]
    frac = torch.tensor([1.0, -1.0, 0.75, -0.5, 0.4375, 0.25, -0.125, 0.0625,
                         0.046875, -0.03125, 0.0, -0.0] + [0.3125] * 20)
    grp = (vmax.unsqueeze(1) * frac.unsqueeze(0)).bfloat16()   # [65280, 32]
    n = grp.shape[0] // 4 * 4
    # four groups per 128-chunk, laid out in fragment order
    x = torch.empty(n // 4, 128, dtype=torch.bfloat16)
    x[:, g.fp4_perm128()] = grp[:n].view(n // 4, 128)
    return x


def _assert_same(x):
    a4, a_s = g.to_fp4_mx(x)
    b4, b_s = g.fp4_mx_spec(x)
    assert torch.equal(a_s, b_s), "scale bytes differ"
    assert torch.equal(a4, b4), "code bytes differ"


def test_spec_every_finite_bf16_max():
    x = all_finite_bf16_as_maxima()
    assert x.shape[0] * 4 >= 65280 - 3
    _assert_same(x)


def test_spec_crafted_rows():
    _assert_same(crafted_rows())


def test_tie_codes_take_lower_code():
    x = crafted_rows()[2:3]
    x4, _ = g.fp4_mx_spec(x)
    codes = torch.stack([x4[0] & 0xF, x4[0] >> 4], dim=1).reshape(-1)[:32]
    # group 0: [6.0, +mids(7), -mids(7), 0, -6.0, mids/2 (7), 0...]
    assert codes[0].item() == 7
    assert codes[1:8].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert codes[8:15].tolist() == [8, 9, 10, 11, 12, 13, 14]
    assert codes[16].item() == 15


def test_negative_zero_code():
    x = crafted_rows()[3:4]
    x4, _ = g.fp4_mx_spec(x)
    assert (x4[0, 0] & 0xF).item() == 8      # -0.01 under max 6.0: code 8


@pytest.mark.parametrize("D", [128, 384, 1024])
def test_spec_random_rows(D):
    gen = torch.Generator().manual_seed(D)
    x = torch.randn(33, D, generator=gen)
    x[5] *= 1e-30
    x[6] *= 1e30
    _assert_same(x.bfloat16())


def test_ingest_is_off_by_default():
    from vainplex_openclaw_amd.pipeline.engine import PipelineConfig

    cfg = PipelineConfig()
    assert cfg.ingest is False
    assert cfg.ingest_capacity == 0
