"""The in-place row-move kernel of forgetting (csrc/index_forget.hip)
against torch indexing on clones of the buffers, compared bitwise over
the whole capacity; consistency of the moved fp4 copy with the quantizer;
and the recall scan seeing the change."""

import pytest
import torch

from test_index_forget import edge_masks
from vainplex_openclaw_amd.ops import gpu as g

pytestmark = pytest.mark.gpu

N, CAP = 1000, 1100
DEV = "cuda:0"


def _buffers(D, cap=CAP, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    index = torch.randint(0, 256, (cap, D * 2), generator=gen, dtype=torch.uint8,
                          device=DEV).view(torch.bfloat16)
    x4 = torch.randint(0, 256, (cap, D // 2), generator=gen, dtype=torch.uint8, device=DEV)
    xs = ((torch.arange(cap * (D // 32), device=DEV) * 7 + 3) % 251).to(torch.uint8)
    xs = xs.view(cap, D // 32)
    owner = torch.arange(cap, dtype=torch.int32, device=DEV)
    sal = (torch.arange(cap, device=DEV).float() + 0.25) / (2 * cap)  # all distinct
    return {"index": index, "X4": x4, "XS": xs, "owner": owner, "salience": sal}


SUBSETS = {
    "all": ("index", "X4", "XS", "owner", "salience"),
    "membrane": ("index", "owner"),
    "pipeline": ("index", "X4", "XS", "salience"),
}


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _run_and_compare(src, dst, bufs, names, good=None):
    """Kernel on `bufs` against clone[dst] = clone[src] over the pairs
    selected by `good` (all by default); the buffers not in `names` must
    not change at all."""
    want = {k: v.clone() for k, v in bufs.items()}
    s, d = src.long(), dst.long()
    if good is not None:
        s, d = s[good], d[good]
    for k in names:
        want[k][d] = want[k][s]
    g.index_move_rows(src, dst, **{k: bufs[k] for k in names})
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(_bits(bufs[k]), _bits(want[k])), k


@pytest.mark.parametrize("D", [128, 512, 1024])
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_move_rows_matches_torch_indexing(D, subset):
    for name, dead in edge_masks(N).items():
        bufs = _buffers(D)
        n_new, dst, src = g.forget_plan(dead.to(DEV))
        assert n_new == N - int(dead.sum())
        _run_and_compare(src, dst, bufs, SUBSETS[subset])


def test_single_row_and_single_pair():
    # n = 1: nothing to move whether the row dies or not
    for dead in (torch.tensor([True]), torch.tensor([False])):
        bufs = _buffers(128, cap=4)
        n_new, dst, src = g.forget_plan(dead.to(DEV))
        assert len(dst) == 0 and n_new == int(not dead[0])
        _run_and_compare(src, dst, bufs, SUBSETS["all"])
    # m = 1: one dead row in front, one live row behind the new end
    dead = torch.zeros(N, dtype=torch.bool)
    dead[17] = True
    for D in (128, 1024):
        bufs = _buffers(D)
        n_new, dst, src = g.forget_plan(dead.to(DEV))
        assert dst.tolist() == [17] and src.tolist() == [N - 1] and n_new == N - 1
        _run_and_compare(src, dst, bufs, SUBSETS["all"])


@pytest.mark.parametrize("D", [128, 1024])
def test_bad_indices_are_skipped(D):
    dead = edge_masks(N)["random0.3"]
    _n_new, dst, src = g.forget_plan(dead.to(DEV))
    src, dst = src.clone(), dst.clone()
    m = len(src)
    assert m > 40
    src[3], src[11], dst[20], dst[31] = -1, CAP, -1, CAP
    src[m - 1], dst[m - 1] = CAP + 5, -7
    good = (src >= 0) & (src < CAP) & (dst >= 0) & (dst < CAP)
    assert int(good.sum()) == m - 5
    _run_and_compare(src, dst, _buffers(D), SUBSETS["all"], good=good)


def test_odd_row_size_takes_torch_indexing():
    """D % 8 != 0 (SalienceIndex allows any dim): same result, no kernel."""
    cap, D = 40, 12
    index = torch.randn(cap, D, device=DEV).bfloat16()
    owner = torch.arange(cap, dtype=torch.int32, device=DEV)
    want = index.clone()
    dead = torch.zeros(30, dtype=torch.bool, device=DEV)
    dead[[1, 4, 29]] = True
    n_new = g.index_forget(dead, index=index, owner=owner)
    assert n_new == 27 and owner[:n_new].tolist()[:5] == [0, 27, 2, 3, 28]
    assert torch.equal(_bits(index[:n_new]), _bits(want[owner[:n_new].long()]))


def test_binding_checks():
    b = _buffers(128)
    i32 = dict(dtype=torch.int32, device=DEV)
    src, dst = torch.tensor([5], **i32), torch.tensor([1], **i32)
    ext = g.ext()
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src, dst)  # no buffer
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src.long(), dst.long(), owner=b["owner"])
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src, torch.tensor([1, 2], **i32), owner=b["owner"])
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src, dst, X4=b["X4"])  # codes without scales
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src, dst, index=b["index"], owner=b["owner"][:-1])
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src, dst, index=b["index"].float())
    with pytest.raises(RuntimeError):
        ext.index_move_rows(src, dst, index=b["index"][:, :64])  # not contiguous


@pytest.fixture(scope="module")
def real_index():
    """A real bf16 index (unit rows) with its MXFP4 copy, D = 512."""
    D = 512
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.nn.functional.normalize(
        torch.randn(CAP, D, generator=gen, device=DEV), dim=1).bfloat16()
    x4, xs = g.quantize_fp4_mx(x)
    return x, x4, xs


def test_moved_fp4_copy_is_the_quantized_index(real_index):
    index, x4, xs = (t.clone() for t in real_index)
    dead = edge_masks(N)["random0.3"].to(DEV)
    n_new = g.index_forget(dead, index=index, X4=x4, XS=xs)
    o4, o_s = g.to_fp4_mx(index[:n_new])
    assert torch.equal(x4[:n_new], o4) and torch.equal(xs[:n_new], o_s)


def test_recall_sees_the_change(real_index):
    orig = real_index[0]
    index, x4, xs = (t.clone() for t in real_index)
    owner = torch.arange(CAP, dtype=torch.int32, device=DEV)
    dead = edge_masks(N)["random0.3"].to(DEV)
    n_new, dst, src = g.forget_plan(dead)
    g.index_move_rows(src, dst, index=index, X4=x4, XS=xs, owner=owner)
    forgotten = torch.nonzero(dead).flatten()[:64]
    moved_from, moved_to = src[:64].long(), dst[:64].long()
    Q = torch.cat([orig[forgotten], orig[moved_from]])
    scores, ids = g.topk_recall_threshold(
        Q, index[:n_new], 4, X4=(x4[:n_new], xs[:n_new]))
    torch.cuda.synchronize()
    # a forgotten row is gone: its best match is what a random unit row
    # gives, |cos| ~ N(0, 1/sqrt(512)); 0.3 is 6.8 sigma
    assert float(scores[:64, 0].max()) < 0.3
    assert int(ids.max()) < n_new
    # a moved row answers under its new id
    assert torch.equal(ids[64:, 0].long(), moved_to)
    assert float(scores[64:, 0].min()) > 0.99
    assert torch.equal(owner[moved_to].long(), moved_from)
