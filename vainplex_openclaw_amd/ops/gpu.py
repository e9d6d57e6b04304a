"""GPU op wrappers: the bridge between the engines and csrc/ kernels.

Every op here REQUIRES the in-tree `_hip_ops` extension when running on a
GPU — there is no silent eager fallback (a GPU box without the extension
raises immediately). CPU reference implementations used by the numerics
tests live in `reference_*` functions.
"""

from __future__ import annotations

import hashlib
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .dfa import MultiDFA
from . import pattern_sets

_EXT = None


def ext():
    """The compiled extension; raises loudly when missing."""
    global _EXT
    if _EXT is None:
        try:
            from .. import _hip_ops  # type: ignore

            _EXT = _hip_ops
        except ImportError as exc:  # pragma: no cover
            raise RuntimeError(
                "vainplex_openclaw_amd._hip_ops is not built. Run "
                "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
                "GPU ops never fall back to eager."
            ) from exc
    return _EXT


def have_ext() -> bool:
    try:
        ext()
        return True
    except RuntimeError:
        return False


# -- message packing --------------------------------------------------------

def pack_messages(messages: Sequence[bytes], device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """Concatenate messages into (bytes u8 [total], offsets i32 [n+1])."""
    offsets = np.zeros(len(messages) + 1, dtype=np.int32)
    for i, m in enumerate(messages):
        offsets[i + 1] = offsets[i] + len(m)
    blob = b"".join(messages)
    b = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    o = torch.from_numpy(offsets)
    if device != "cpu":
        b = b.to(device, non_blocking=True)
        o = o.to(device, non_blocking=True)
    return b, o


# -- DFA scan ---------------------------------------------------------------

class DeviceDFA:
    """Packed MultiDFA tables resident on one device."""

    def __init__(self, mdfa: MultiDFA, device) -> None:
        packed = mdfa.pack()
        self.next = torch.from_numpy(packed["next"].view(np.int16)).to(device)
        self.accept = torch.from_numpy(packed["accept"].view(np.int64)).to(device)
        self.eof = torch.from_numpy(packed["eof"].view(np.int64)).to(device)
        self.class_maps = torch.from_numpy(packed["class_maps"].reshape(-1)).to(device)
        self.meta = torch.from_numpy(packed["meta"].reshape(-1)).to(device)
        self.n_dfas = packed["meta"].shape[0]
        self.mdfa = mdfa


_device_dfas: Dict[Tuple[str, int], DeviceDFA] = {}


def device_family(name: str, device) -> DeviceDFA:
    dev = torch.device(device)
    key = (name, dev.index if dev.index is not None else -1)
    if key not in _device_dfas:
        _device_dfas[key] = DeviceDFA(pattern_sets.get_family(name), dev)
    return _device_dfas[key]


def dfa_scan(bytes_t: torch.Tensor, offsets: torch.Tensor, family: str) -> torch.Tensor:
    """Per-message u64 hit masks (as int64 tensor) for one pattern family."""
    d = device_family(family, bytes_t.device)
    meta2d = d.meta.view(d.n_dfas, 4)
    return ext().dfa_scan(bytes_t, offsets, d.next, d.accept, d.eof, d.class_maps, meta2d)


def reference_dfa_scan(messages: Sequence[bytes], family: str) -> np.ndarray:
    mdfa = pattern_sets.get_family(family)
    return np.array([mdfa.scan(m) for m in messages], dtype=np.uint64).view(np.int64)


# -- SHA-256 / Merkle -------------------------------------------------------

def sha256_leaves(bytes_t: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    return ext().sha256_leaves(bytes_t, offsets)


def merkle_root(digests: torch.Tensor) -> torch.Tensor:
    return ext().merkle_root(digests)


def reference_sha256_leaves(messages: Sequence[bytes]) -> np.ndarray:
    return np.stack([np.frombuffer(hashlib.sha256(m).digest(), dtype=np.uint8) for m in messages])


def reference_merkle_root(messages: Sequence[bytes]) -> bytes:
    from ..governance.audit import merkle_root as cpu_root

    return bytes.fromhex(cpu_root(list(messages)))


# -- encoder ----------------------------------------------------------------

def encode_messages(
    bytes_t: torch.Tensor, offsets: torch.Tensor, embed: torch.Tensor, normalize: bool = True
) -> torch.Tensor:
    return ext().encode_messages(bytes_t, offsets, embed, normalize)


def reference_encode(messages: Sequence[bytes], embed: np.ndarray, normalize: bool = True) -> np.ndarray:
    """CPU reference of csrc/encoder.hip (fnv1a 4-gram, stride-subsampled
    mean, L2 norm)."""
    vocab, dim = embed.shape
    out = np.zeros((len(messages), dim), dtype=np.float32)
    max_tokens = 512
    for i, m in enumerate(messages):
        n_pos = max(len(m) - 3, 0)
        stride = max((n_pos + max_tokens - 1) // max_tokens, 1)
        toks = []
        for t in range((n_pos + stride - 1) // stride if n_pos else 0):
            p = t * stride
            h = 2166136261
            for b in m[p : p + 4]:
                h = ((h ^ b) * 16777619) & 0xFFFFFFFF
            toks.append(h & (vocab - 1))
        if toks:
            f = embed[toks].astype(np.float32).mean(axis=0)
        else:
            f = np.zeros(dim, dtype=np.float32)
        if normalize:
            n = np.sqrt(max((f * f).sum(), 1e-12))
            f = f / n
        out[i] = f
    return out


# -- GEMM / top-k -----------------------------------------------------------

def gemm_nt(
    A: torch.Tensor,
    B: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    act: int = 0,
    out_bf16: bool = False,
) -> torch.Tensor:
    return ext().gemm_nt(A, B, bias, act, out_bf16)


def _owner_args(owner, qowner):
    """Both or neither; int32 contiguous for the kernels."""
    if (owner is None) != (qowner is None):
        raise ValueError("owner and qowner must be given together")
    if owner is None:
        return None, None
    return owner.to(torch.int32).contiguous(), qowner.to(torch.int32).contiguous()


def topk_recall(
    Q: torch.Tensor,
    X: torch.Tensor,
    k: int,
    n_swaths: int = 0,
    owner: Optional[torch.Tensor] = None,
    qowner: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cosine top-k of each Q row against X (csrc/topk_recall.hip v3).

    Swath count: a multiple of 8 (XCD-aware grid mapping), sized so
    qblocks*swaths fills the 256 CUs, capped by the merge kernel's
    n_swaths*k <= 1024 register budget and the index size.

    `owner` (int32 [nx], values >= 0) and `qowner` (int32 [nq]) turn on the
    in-kernel isolation filter: query q sees row j only if qowner[q] < 0 or
    owner[j] == qowner[q]. A query with fewer than k eligible rows returns
    id -1 / score -1e30 in the unfilled slots.
    """
    owner, qowner = _owner_args(owner, qowner)
    if n_swaths <= 0:
        qblocks = (Q.shape[0] + 255) // 256  # BM=256
        want = max(1, 256 // max(qblocks, 1))
        n_swaths = max(8, (want // 8) * 8)
        n_swaths = min(n_swaths, (1024 // max(k, 1)) // 8 * 8)
        n_swaths = min(n_swaths, max(1, X.shape[0] // 256))
        n_swaths = max(1, n_swaths)
    if owner is None:
        s, i = ext().topk_recall(Q, X, k, n_swaths)
    else:
        s, i = ext().topk_recall(Q, X, k, n_swaths, xowner=owner, qowner=qowner)
    return s, i


def reference_owned_topk(
    Q: torch.Tensor,
    X: torch.Tensor,
    k: int,
    owner: torch.Tensor,
    qowner: torch.Tensor,
    salience: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 masked dense reference of the owner-filtered recall: mask the
    ineligible (query, row) pairs, THEN take the top-k. Runs on any device,
    CPU tensors included. Slots past a query's eligible rows hold id -1 /
    score -1e30, like the kernels."""
    scores = Q.float() @ X.float().T
    if salience is not None:
        scores = scores * salience.float().unsqueeze(0)
    qo = qowner.long().unsqueeze(1)
    eligible = (qo < 0) | (owner.long().unsqueeze(0) == qo)
    scores = torch.where(eligible, scores, torch.full_like(scores, -1e30))
    kk = min(k, X.shape[0])
    top = torch.topk(scores, kk, dim=1)
    ids = torch.where(top.values > -1e29, top.indices,
                      torch.full_like(top.indices, -1)).to(torch.int32)
    vals = top.values
    if kk < k:
        pad = (Q.shape[0], k - kk)
        vals = torch.cat([vals, vals.new_full(pad, -1e30)], dim=1)
        ids = torch.cat([ids, ids.new_full(pad, -1)], dim=1)
    return vals, ids


def owned_thresholds(
    mu: torch.Tensor,
    sigma: torch.Tensor,
    n_owned: torch.Tensor,
    target_candidates: int,
    z_margin: float = 0.0,
) -> torch.Tensor:
    """Per-query scan thresholds under the owner filter. Query q competes
    among its owner's n_owned[q] rows only, so its Gaussian tail probability
    is p = clamp(target_candidates / n_owned, 1e-12, 0.5) and theta = mu +
    sigma * (z(p) - z_margin) with z(p) = sqrt(2) * erfinv(1 - 2p). A query
    whose owner has no rows gets +inf (nothing can be appended). Device
    agnostic (CPU tensors included)."""
    n = n_owned.to(torch.float64)
    p = (float(target_candidates) / n.clamp_min(1.0)).clamp(1e-12, 0.5)
    z = (math.sqrt(2.0) * torch.erfinv(1.0 - 2.0 * p) - z_margin).to(mu.dtype)
    theta = mu + sigma * z
    return torch.where(n_owned > 0, theta, torch.full_like(theta, float("inf")))


def to_fp8_bytes(x: torch.Tensor, scale: float = 8.0) -> torch.Tensor:
    """bf16 -> e4m3 bytes, pre-scaled so typical unit-vector components
    (~N(0, 1/sqrt(D))) land in e4m3's normal range."""
    return (x.float() * scale).to(torch.float8_e4m3fn).view(torch.uint8)


_E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def fp4_perm128() -> torch.Tensor:
    """Element order the v_mfma_scale..f8f6f4 fp4 B operand expects, per
    128-k chunk (probed on hardware, tools/probe_fp4map.hip): LDS slot g
    (= lane kgrp g) holds k in {base, base+32} + [0,16) with base =
    (g&1)*64 + (g>>1)*16, packed two-per-byte (low nibble = even
    position). A lane's 32 elements share ONE e8m0 scale, so scale
    groups are 32 consecutive elements in THIS order."""
    base = torch.arange(16)
    order = []
    for g in range(4):
        s = (g & 1) * 64 + (g >> 1) * 16
        order.append(s + base)
        order.append(s + 32 + base)
    return torch.cat(order)


def to_fp4_mx(x: torch.Tensor, chunk_rows: int = 1_048_576) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 [N, D] -> MXFP4 in the hardware fragment order: packed e2m1
    nibbles [N, D/2] + per-lane-group e8m0 scales [N, D/32]. The e8m0
    exponent maps each group's max |v| onto e2m1's top code (6.0)."""
    N, D = x.shape
    assert D % 128 == 0
    mids = torch.tensor(_E2M1_MIDPOINTS, device=x.device)
    p128 = fp4_perm128().to(x.device)
    perm = (torch.arange(0, D, 128, device=x.device).unsqueeze(1) + p128.unsqueeze(0)).reshape(-1)
    out4 = torch.empty((N, D // 2), dtype=torch.uint8, device=x.device)
    outs = torch.empty((N, D // 32), dtype=torch.uint8, device=x.device)
    for r0 in range(0, N, chunk_rows):
        v = x[r0:r0 + chunk_rows].float()[:, perm].view(-1, D // 32, 32)
        amax = v.abs().amax(dim=2, keepdim=True)
        e = torch.where(amax > 0, (amax / 6.0).log2().ceil(), torch.zeros_like(amax))
        e = e.clamp(-127, 127)
        outs[r0:r0 + chunk_rows] = (e.squeeze(2) + 127).to(torch.uint8)
        y = v * torch.exp2(-e)
        code = torch.bucketize(y.abs().contiguous(), mids).to(torch.uint8)
        code |= (y < 0).to(torch.uint8) << 3
        code = code.view(-1, D)
        out4[r0:r0 + chunk_rows] = code[:, 0::2] | (code[:, 1::2] << 4)
    return out4, outs


def fp4_mx_spec(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The contract of csrc/fp4_quantize.hip written down in torch: the
    same output as to_fp4_mx, bit for bit on finite input, from integer
    rules only (no log2, no permutation gather). Device agnostic.

    Per 128-element chunk c and group g in 0..3 the group's 32 elements
    are c*128 + s + [0,16) and c*128 + s + 32 + [0,16), s = (g&1)*64 +
    (g>>1)*16; their codes fill bytes c*64 + g*16 + [0,16) (low nibble =
    even position) and their scale is XS[:, c*4 + g].

    Scale: the group max as a bf16 bit pattern has exponent field E and
    mantissa M. max == 0 -> e = 0; else e = E - 129 if M <= 64 (max <=
    1.5 * 2^(E-127)) else E - 128, clamped below at -127 (which also
    covers a subnormal max, E = 0). Scale byte = e + 127.
    Code: y = v * 2^-e (exact); magnitude code = number of e2m1 midpoints
    strictly below |y|; sign bit iff y < 0 in fp32."""
    N, D = x.shape
    assert D % 128 == 0 and x.dtype == torch.bfloat16
    # element c*128 + (g&1)*64 + half*32 + (g>>1)*16 + i: split the chunk
    # into (g&1, half, g>>1, i) and reorder to (g>>1, g&1, half, i), i.e.
    # group-major with 32 consecutive elements per group
    def grouped(t):
        t = t.view(N, D // 128, 2, 2, 2, 16).permute(0, 1, 4, 2, 3, 5)
        return t.reshape(N, D // 32, 32)

    x = x.contiguous()
    b = grouped(x.view(torch.int16).to(torch.int32))
    v = grouped(x.float())
    amax = (b & 0x7FFF).amax(dim=2)
    E, M = amax >> 7, amax & 0x7F
    e = torch.where(M <= 64, E - 129, E - 128).clamp_min(-127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    outs = (e + 127).to(torch.uint8)
    inv = ((127 - e) << 23).to(torch.int32).view(torch.float32)  # 2^-e
    y = v * inv.unsqueeze(2)
    a = y.abs()
    code = torch.zeros_like(b)
    for mid in _E2M1_MIDPOINTS:
        code += (a > mid).to(torch.int32)
    code |= (y < 0).to(torch.int32) << 3
    code = code.view(N, D)
    out4 = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    return out4, outs


_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def reference_fp4_decode(P4: torch.Tensor, S: torch.Tensor,
                         natural_order: bool = False) -> torch.Tensor:
    """MXFP4 rows back to numbers, in fp64 [n, D]: P4 = packed e2m1
    nibbles [n, D/2] (low nibble = even position), S = e8m0 scales
    [n, D/32]. Nibble = sign bit, then an index into the e2m1 grid; byte
    j's two elements are times 2^(S[:, j // 16] - 127). Every value is
    exact in fp64. The result is in the stored (fragment) order of
    to_fp4_mx; natural_order=True undoes fp4_perm128 per 128-chunk.
    Plain torch, device agnostic, independent of the extension."""
    n, half = P4.shape
    D = half * 2
    assert P4.dtype == torch.uint8 and S.dtype == torch.uint8
    assert S.shape == (n, D // 32)
    grid = torch.tensor(_E2M1_GRID, dtype=torch.float64, device=P4.device)
    codes = torch.stack([P4 & 0xF, P4 >> 4], dim=2).reshape(n, D).long()
    mag = grid[codes & 7]
    val = torch.where(codes >= 8, -mag, mag)
    scale = torch.exp2(S.to(torch.float64) - 127.0).repeat_interleave(32, dim=1)
    dec = val * scale
    if not natural_order:
        return dec
    p128 = fp4_perm128().to(P4.device)
    perm = (torch.arange(0, D, 128, device=P4.device).unsqueeze(1) + p128.unsqueeze(0)).reshape(-1)
    out = torch.empty_like(dec)
    out[:, perm] = dec
    return out


def reference_scores_bound(q: torch.Tensor, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp64 q @ x.T of two decoded operands [nq, D], [nx, D] and the
    per-cell bound an fp32-accumulating kernel must stay inside:
    D * 2^-22 * sum_i |q_i| |x_i|. At most D additions, each rounding or
    truncating by at most 2^-23 relative to a partial sum that
    sum |q_i||x_i| bounds, times 2 for the undocumented alignment inside
    the 128-wide MFMA add. A derived worst case, not a measured figure."""
    D = q.shape[1]
    ref = q @ x.T
    bound = (q.abs() @ x.abs().T) * (D * 2.0 ** -22)
    return ref, bound


def reference_fp4x4_scores(Q4: torch.Tensor, QS: torch.Tensor, X4: torch.Tensor,
                           XS: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """What an fp4 x fp4 scan score is supposed to be: (ref, bound), both
    fp64 [nq, nx] (reference_scores_bound of the decoded operands). Q and X
    are stored in the same fragment order, so no permutation is needed."""
    return reference_scores_bound(reference_fp4_decode(Q4, QS),
                                  reference_fp4_decode(X4, XS))


def quantize_fp4_mx(
    x: torch.Tensor,
    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """to_fp4_mx as ONE kernel launch (csrc/fp4_quantize.hip): bf16 [n, D]
    read once, codes and scales written once, no fp32 temporaries. Output
    is bit-for-bit to_fp4_mx(x). `out` = (X4 [n, D/2], XS [n, D/32])
    fills preallocated contiguous rows in place of allocating."""
    x = x.contiguous()
    if out is None:
        x4, xs = ext().quantize_fp4_mx(x)
    else:
        x4, xs = ext().quantize_fp4_mx(x, out[0], out[1])
    return x4, xs


def index_append(
    feats: torch.Tensor,
    src_idx: Optional[torch.Tensor],
    dst_row0: int,
    index: torch.Tensor,
    X4: Optional[torch.Tensor] = None,
    XS: Optional[torch.Tensor] = None,
    owner_dst: Optional[torch.Tensor] = None,
    owner_src: Optional[torch.Tensor] = None,
    salience_dst: Optional[torch.Tensor] = None,
    salience_init: float = 1.0,
    id_dst: Optional[torch.Tensor] = None,
    id_base: int = 0,
) -> None:
    """Append rows to a live recall index in one launch: row dst_row0 + i
    of `index` (bf16 [cap, D]), of the MXFP4 pair X4/XS, of `owner_dst`
    and of `salience_dst` receives feats[src_idx[i]] (feats[i] when
    src_idx is None), its fp4 codes and scales (as to_fp4_mx would build
    them), owner_src[src_idx[i]] and salience_init; row dst_row0 + i of
    `id_dst` (int64 [cap]) receives id_base + src_idx[i], the row's memory
    id. Every destination except `index` is optional. A src_idx entry
    outside feats leaves its destination row untouched; dst_row0 + n past
    the capacity raises."""
    if id_dst is None:
        ext().index_append(feats, src_idx, int(dst_row0), index, X4, XS,
                           owner_dst, owner_src, salience_dst, float(salience_init))
    else:
        ext().index_append(feats, src_idx, int(dst_row0), index, X4, XS,
                           owner_dst, owner_src, salience_dst, float(salience_init),
                           id_dst, int(id_base))


def evict_mask(salience: torch.Tensor, count: int) -> torch.Tensor:
    """bool[n] marking exactly min(max(count, 0), n) rows of `salience`
    (fp32 [n]), the lowest ones. Deterministic: with v the count-th
    smallest value every row with s < v is marked, and among the rows with
    s == v the lowest row indices until the count is reached. Ties are the
    normal case (rows ingested in one step and never recalled share a value
    bit for bit, and so do all rows at the floor). Pure torch, no host
    read; runs on CPU tensors too."""
    n = salience.numel()
    c = min(max(int(count), 0), n)
    if c == 0:
        return torch.zeros(n, dtype=torch.bool, device=salience.device)
    if c == n:
        return torch.ones(n, dtype=torch.bool, device=salience.device)
    v = torch.topk(salience, c, largest=False, sorted=False).values.max()
    below = salience < v
    tie = salience == v
    room = c - below.sum()
    # 1-based rank of a tie among the ties, by row index
    rank = torch.cumsum(tie, dim=0, dtype=torch.int32)
    return below | (tie & (rank <= room))


def forget_plan(dead: torch.Tensor) -> Tuple[int, torch.Tensor, torch.Tensor]:
    """The compaction rule of forgetting (hole filling). `dead` is bool[n]
    over the live rows; with n_new = n - dead.sum(), dst is the dead rows
    below n_new and src the live rows at or above n_new, both ascending
    int32 and equally long. Moving row src[j] onto row dst[j] for every j
    makes [:n_new] the live rows. Sources and destinations are disjoint and
    the destinations unique, so the moves need no order. At most
    min(#dead, n_new) rows move.

    Row order is NOT preserved: a survivor from the tail lands in a hole.
    Nothing depends on row order; salience carries age.

    n_new is the one value read back to the host (the two nonzero() calls
    size their outputs from the same mask)."""
    n = dead.numel()
    n_new = n - int(dead.sum())
    dst = torch.nonzero(dead[:n_new]).flatten().to(torch.int32)
    src = (torch.nonzero(~dead[n_new:]).flatten() + n_new).to(torch.int32)
    return n_new, dst, src


def index_move_rows(
    src: torch.Tensor,
    dst: torch.Tensor,
    index: Optional[torch.Tensor] = None,
    X4: Optional[torch.Tensor] = None,
    XS: Optional[torch.Tensor] = None,
    owner: Optional[torch.Tensor] = None,
    salience: Optional[torch.Tensor] = None,
    ids: Optional[torch.Tensor] = None,
) -> None:
    """Row dst[j] of every given buffer takes the contents of row src[j],
    bitwise and in place, in one launch (csrc/index_forget.hip). `index`
    is bf16 [cap, D], X4/XS the MXFP4 pair, owner int32 [cap], salience
    fp32 [cap], ids int64 [cap]; any subset, at least one. dst must be unique and disjoint
    from src (forget_plan's lists are). The kernel skips a pair with an
    index outside [0, cap). CPU tensors, and a bf16 row that is not a
    multiple of 16 bytes (D % 8 != 0), take torch indexing instead."""
    bufs = [b for b in (index, X4, XS, owner, salience, ids) if b is not None]
    if not bufs:
        raise ValueError("index_move_rows needs at least one buffer")
    if src.numel() == 0:
        return
    on_gpu = src.is_cuda and all(b.is_cuda for b in bufs)
    if on_gpu and (index is None or index.shape[1] % 8 == 0):
        ext().index_move_rows(src, dst, index, X4, XS, owner, salience, ids)
        return
    s, d = src.long(), dst.long()
    for b in bufs:
        b[d] = b[s]


def index_forget(
    dead: torch.Tensor,
    index: Optional[torch.Tensor] = None,
    X4: Optional[torch.Tensor] = None,
    XS: Optional[torch.Tensor] = None,
    owner: Optional[torch.Tensor] = None,
    salience: Optional[torch.Tensor] = None,
    ids: Optional[torch.Tensor] = None,
) -> int:
    """Forget the live rows marked in `dead` (bool[n], n = live rows):
    forget_plan, then one index_move_rows over the given buffers. Returns
    n_new; the live rows are then [:n_new] of every buffer and the
    contents of rows >= n_new are unspecified."""
    n_new, dst, src = forget_plan(dead)
    index_move_rows(src, dst, index=index, X4=X4, XS=XS, owner=owner, salience=salience,
                    ids=ids)
    return n_new


# -- memory ids: rows by id (csrc/index_ids.hip) -----------------------------

FIND_CHUNK = 4096  # wanted ids per launch: 32 KB of LDS


def reference_find_rows(ids_col: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """The rule of find_rows in torch, on any device: int32 [len(want)],
    the row of `ids_col` (int64 [n], the live prefix of the ids column)
    holding each wanted id, or -1. A negative id is never found, on either
    side; of several rows holding one id the highest wins. A stable sort
    keeps equal ids in row order, so the last of a run (searchsorted
    right=True, minus one) is the highest row."""
    want = want.to(torch.int64)
    out = torch.full((want.numel(),), -1, dtype=torch.int32, device=ids_col.device)
    if ids_col.numel() == 0 or want.numel() == 0:
        return out
    vals, order = torch.sort(ids_col, stable=True)
    pos = torch.searchsorted(vals, want, right=True) - 1
    posc = pos.clamp_min(0)
    hit = (pos >= 0) & (vals[posc] == want) & (want >= 0)
    return torch.where(hit, order[posc].to(torch.int32), out)


def find_rows(ids_col: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """int32 [len(want)]: the row of `ids_col` (int64 [n], the live prefix
    index_ids[:n_rows]) that holds each wanted id, -1 where none does.
    `want` is int64 in any order and may repeat ids; negative ids are never
    found; of several rows holding one id the highest wins
    (reference_find_rows is the same rule in torch, and the CPU path).

    One pass over the column per FIND_CHUNK wanted ids
    (csrc/index_ids.hip): the sorted, distinct ids of a chunk sit in LDS and
    every row is searched there, so nothing of the column's size is
    allocated. torch.unique sizes its result on the host; that is the one
    host read."""
    if not ids_col.is_cuda:
        return reference_find_rows(ids_col, want)
    want = want.to(device=ids_col.device, dtype=torch.int64).contiguous()
    m = want.numel()
    if ids_col.numel() == 0 or m == 0:
        return torch.full((m,), -1, dtype=torch.int32, device=ids_col.device)
    uniq, inv = torch.unique(want, return_inverse=True)
    rows = torch.full((uniq.numel(),), -1, dtype=torch.int32, device=ids_col.device)
    col = ids_col.contiguous()
    for c0 in range(0, uniq.numel(), FIND_CHUNK):
        ext().index_find_ids(col, uniq[c0:c0 + FIND_CHUNK], rows[c0:c0 + FIND_CHUNK])
    return rows[inv]


# -- ingest dedup: near-duplicate detection (csrc/ingest_dedup.hip) ----------
#
# Similarity is the plain dot product of bf16 feature rows, which is what
# recall scores: rows are not re-normalised, so two identical messages score
# |f|^2, a few 1e-3 below 1. The kernels and the torch path accumulate in
# fp32, the reference_* twins in fp64; they agree wherever no compared pair
# lies within the fp32 accumulation error (about D * 2^-24) of tau.

def _first_similar(S: torch.Tensor, elig: torch.Tensor, tau: float,
                   owner: Optional[torch.Tensor]) -> torch.Tensor:
    B = S.shape[0]
    ar = torch.arange(B, device=S.device)
    e = elig.bool()
    ok = (S >= tau) & (ar.unsqueeze(0) < ar.unsqueeze(1)) & e.unsqueeze(1) & e.unsqueeze(0)
    if owner is not None:
        ok &= owner.unsqueeze(1) == owner.unsqueeze(0)
    j = torch.where(ok, ar.unsqueeze(0), torch.full_like(ar, B).unsqueeze(0)).min(dim=1).values
    first = torch.where(j < B, j, ar)
    return torch.where(e, first, torch.full_like(first, -1)).to(torch.int32)


def reference_batch_first_similar(F: torch.Tensor, elig: torch.Tensor, tau: float,
                                  owner: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The batch rule of ingest dedup, dots in fp64: for an eligible row i,
    first[i] is the smallest eligible j < i with owner[j] == owner[i] (when
    owners are given) and dot(F_i, F_j) >= tau, or i itself if there is
    none; first[i] = -1 for an ineligible i. Row i is stored iff first[i]
    == i. Single link: a dropped row is within tau of an EARLIER ELIGIBLE
    row, which may itself have been dropped."""
    Fd = F.detach().cpu().double()
    own = None if owner is None else owner.detach().cpu()
    return _first_similar(Fd @ Fd.T, elig.detach().cpu(), float(tau), own)


def batch_first_similar(F: torch.Tensor, elig: torch.Tensor, tau: float,
                        owner: Optional[torch.Tensor] = None) -> torch.Tensor:
    """reference_batch_first_similar with fp32 accumulation, int32 [B]: one
    launch of batch_first_similar_kernel (F . F^T over the lower triangle
    on the bf16 MFMA, min j reduced in the block, one atomicMin per row and
    block). F is bf16 [B, D], D % 32 == 0; elig bool [B]; owner int32 [B]
    or None. CPU tensors take a torch path."""
    B = F.shape[0]
    if not F.is_cuda:
        Ff = F.float()
        return _first_similar(Ff @ Ff.T, elig, float(tau), owner)
    elig = elig.bool().contiguous()
    ar = torch.arange(B, dtype=torch.int32, device=F.device)
    first = torch.where(elig, ar, torch.full_like(ar, -1))
    if owner is not None:
        owner = owner.to(torch.int32).contiguous()
    ext().batch_first_similar(F.contiguous(), elig, float(tau), owner, first)
    return first


def _dup_rows(F: torch.Tensor, ids: torch.Tensor, X: torch.Tensor, tau: float,
              xowner: Optional[torch.Tensor], qowner: Optional[torch.Tensor]
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    B, n = F.shape[0], X.shape[0]
    idl = ids.long()
    if n == 0 or idl.shape[1] == 0:
        return (torch.full((B,), -1, dtype=torch.int32, device=F.device),
                torch.full((B,), -math.inf, dtype=F.dtype, device=F.device))
    ok = (idl >= 0) & (idl < n)
    safe = idl.clamp(0, n - 1)
    dots = (X[safe] * F.unsqueeze(1)).sum(dim=2)
    if xowner is not None:
        ok &= xowner[safe] == qowner.unsqueeze(1)
    dots = torch.where(ok & (dots >= tau), dots, torch.full_like(dots, -math.inf))
    best = dots.max(dim=1).values
    found = best > -math.inf
    # equal dots go to the lowest id
    tie = torch.where((dots == best.unsqueeze(1)) & found.unsqueeze(1), idl,
                      torch.full_like(idl, n))
    row = torch.where(found, tie.min(dim=1).values, torch.full_like(best, -1, dtype=torch.long))
    return row.to(torch.int32), best


def reference_recall_dup_rows(F: torch.Tensor, ids: torch.Tensor, X: torch.Tensor,
                              tau: float, xowner: Optional[torch.Tensor] = None,
                              qowner: Optional[torch.Tensor] = None
                              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The index rule of ingest dedup, dots in fp64: dup_row[i] is the row
    among ids[i, :] with the largest dot(F_i, X_row) >= tau, equal dots
    going to the lowest id, or -1. An id outside [0, len(X)) is skipped
    (-1 = unfilled slot, stale, or another rank's row), and with owners so
    is a row whose xowner differs from qowner[i]. dup_dot is that dot,
    undefined where dup_row < 0. Only recalled rows are looked at."""
    c = lambda t: None if t is None else t.detach().cpu()
    return _dup_rows(F.detach().cpu().double(), ids.detach().cpu(),
                     X.detach().cpu().double(), float(tau), c(xowner), c(qowner))


def recall_dup_rows(F: torch.Tensor, ids: torch.Tensor, X: torch.Tensor, tau: float,
                    xowner: Optional[torch.Tensor] = None,
                    qowner: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """reference_recall_dup_rows with fp32 accumulation, (int32 [B], fp32
    [B]): one launch of recall_dup_rows_kernel (a wave per message, query
    row in registers, candidates gathered with 16-byte loads). F bf16
    [B, D], ids int [B, k], X bf16 [n, D], D % 8 == 0 and D <= 2048;
    xowner int32 [n] and qowner int32 [B] go together. The kernel checks
    every id against [0, n) before it loads through it. CPU tensors take a
    torch path."""
    if (xowner is None) != (qowner is None):
        raise ValueError("recall_dup_rows: xowner and qowner go together")
    if not F.is_cuda:
        return _dup_rows(F.float(), ids, X.float(), float(tau), xowner, qowner)
    if xowner is not None:
        xowner = xowner.to(torch.int32).contiguous()
        qowner = qowner.to(torch.int32).contiguous()
    row, dot = ext().recall_dup_rows(F.contiguous(), ids.to(torch.int32).contiguous(),
                                     X.contiguous(), float(tau), xowner, qowner)
    return row, dot


def topk_recall_fp8(Q8: torch.Tensor, X8: torch.Tensor, k: int, n_swaths: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stage-1 fp8 scan: candidate ids ranked by e4m3 cosine (csrc
    topk_recall_fp8_kernel). Inputs are uint8 views of e4m3 bytes."""
    if n_swaths <= 0:
        qblocks = (Q8.shape[0] + 255) // 256
        want = max(1, 256 // max(qblocks, 1))
        n_swaths = max(8, (want // 8) * 8)
        n_swaths = min(n_swaths, (1024 // max(k, 1)) // 8 * 8)
        n_swaths = min(n_swaths, max(1, X8.shape[0] // 256))
        n_swaths = max(1, n_swaths)
    s, i = ext().topk_recall_fp8(Q8, X8, k, n_swaths)
    return s, i


def topk_recall_two_stage(
    Q: torch.Tensor,
    X: torch.Tensor,
    X8: torch.Tensor,
    k: int,
    overfetch: int = 2,
    salience: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two-stage exact-rescore recall: fp8 scan of the full index for
    k*overfetch candidates (half the staged bytes of the bf16 scan = the
    measured GLDS transport bound), then exact bf16/fp32 rescore of the
    candidates and final top-k. Final scores are EXACT cosines; stage-1
    only has to keep the true top-k inside the candidate set (error
    sigma ~0.003 vs candidate margins ~10x that).
    """
    k2 = min(32, max(k * overfetch, k))  # TOPK_MAX LDS bound in the scan kernel
    Q8 = to_fp8_bytes(Q)
    _s8, ids8 = topk_recall_fp8(Q8, X8, k2)
    ids = ids8.long().clamp_min(0)  # -1 slots -> row 0 (rescored, never top)
    cand = X[ids]  # [nq, k2, D] bf16 gather
    exact = torch.einsum("qd,qkd->qk", Q.float(), cand.float())
    if salience is not None:
        exact = exact * salience[ids]
    exact = torch.where(ids8 < 0, torch.full_like(exact, -1e30), exact)
    top = torch.topk(exact, k, dim=1)
    return top.values, torch.gather(ids8, 1, top.indices)


def edit_distance_batch(pairs: Sequence[Tuple[bytes, bytes]], device="cuda") -> torch.Tensor:
    """Batched Levenshtein over (a, b) byte-string pairs (csrc
    edit_distance_kernel, one 64-lane wave per pair, anti-diagonal DP).
    Inputs are capped at 512 bytes each — the doom-loop detector caps
    commands at 500 chars (SURVEY §2.8 / reference doom-loop.ts:76-90)."""
    flat: list = []
    for a, b in pairs:
        flat.append(a[:512])
        flat.append(b[:512])
    if not flat:
        return torch.empty(0, dtype=torch.int32)
    bytes_t, offsets = pack_messages(flat, device=device)
    return ext().edit_distance(bytes_t, offsets)


def reference_edit_distance(a: bytes, b: bytes) -> int:
    """Plain CPU Levenshtein for the numerics tests."""
    la, lb = len(a), len(b)
    prev = list(range(lb + 1))
    for i in range(1, la + 1):
        cur = [i] + [0] * lb
        for j in range(1, lb + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1,
                         prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[lb]


# -- firewall tail ----------------------------------------------------------

def firewall_verdict(
    inj_hits: torch.Tensor,
    red_hits: torch.Tensor,
    logits: torch.Tensor,
    agent_idx: torch.Tensor,
    agent_trust: torch.Tensor,
    tool_risk: torch.Tensor,
    freq_count: torch.Tensor,
    hour: int,
    n_agents: int,
    cred_bits: int = pattern_sets.REDACTION_CREDENTIAL_BITS,
    inj_threshold: float = 0.9,
):
    v, r, sd, vd = ext().firewall_verdict(
        inj_hits, red_hits, logits, agent_idx, agent_trust, tool_risk, freq_count,
        hour, cred_bits, inj_threshold, n_agents,
    )
    return v, r, sd, vd


def trust_recompute(state: Dict[str, torch.Tensor], sdelta: torch.Tensor, vdelta: torch.Tensor) -> None:
    ext().trust_recompute(
        state["success"], state["violation"], sdelta, vdelta,
        state["age_days"], state["clean_streak"], state["manual_adj"], state["score"],
    )


def audit_pack(
    verdict: torch.Tensor, risk: torch.Tensor, inj_hits: torch.Tensor, red_hits: torch.Tensor,
    agent_idx: torch.Tensor, agent_trust: torch.Tensor, inj_score: torch.Tensor,
    ts_ms: int, msg_id0: int, batch_seq: int,
) -> torch.Tensor:
    return ext().audit_pack(
        verdict, risk, inj_hits, red_hits, agent_idx, agent_trust, inj_score,
        ts_ms, msg_id0, batch_seq,
    )


HIST_NB = 256  # csrc/topk_recall.hip HIST_NB


def hist_edges(theta: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[nq, HIST_NB + 1] fp32 bin edges of the dropped-hit histogram:
    edge(j) = fp32(fp64(j) * fp64(w) + fp64(theta)). edge(HIST_NB) bounds
    nothing (the last bin is open above); it is there so that edge(b + 1)
    exists for every bin."""
    j = torch.arange(HIST_NB + 1, dtype=torch.float64, device=theta.device)
    e = j.unsqueeze(0) * w.double().unsqueeze(1) + theta.double().unsqueeze(1)
    return e.float()


def hist_bin_spec(v: torch.Tensor, theta: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The bin rule of the hist scan kernels (csrc/topk_recall.hip hist_bin),
    bit for bit, in torch; device agnostic (CPU tensors included). `v` is
    [nq, n] fp32 scores above theta, `theta` and `w` are [nq] fp32, w > 0.
    Returns int64 bins in [0, HIST_NB).

    bin(v) is the b with edge(b) < v <= edge(b + 1) (hist_edges); bin 0 also
    takes everything down to theta and the last bin is open above. The bin
    is estimated from (v - theta) * (1 / w), clamped as a float ahead of the
    int conversion (fmax drops a NaN, fmin an inf), then moved by at most one
    bin against edge(b) and edge(b + 1). The estimate is within one bin of
    the rule as long as w spans a few ulps of theta and of the scores; for a
    smaller w the result is still this function's, in the kernel too, but
    neighbouring edges coincide and the rule above has no single answer."""
    v = v.float()
    th = theta.float().unsqueeze(1)
    inv_w = (1.0 / w.float()).unsqueeze(1)
    t = (v - th) * inv_w
    t = torch.fmin(torch.fmax(t, t.new_zeros(())), t.new_full((), float(HIST_NB - 1)))
    b = t.to(torch.int64)
    edges = hist_edges(theta.float(), w.float())
    lo = edges.gather(1, b)
    hi = edges.gather(1, b + 1)
    down = (b > 0) & ~(v > lo)
    up = ~down & (b < HIST_NB - 1) & (v > hi)
    return b - down.long() + up.long()


def overflow_rescan_plan(
    cand_scores: torch.Tensor,
    counts: torch.Tensor,
    hist: torch.Tensor,
    theta: torch.Tensor,
    w: torch.Tensor,
    cap: int,
    need,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Where to rescan the queries that overflowed their candidate buffer.
    Inputs are the outputs of the hist scan (topk_scan_threshold_fp4x4_hist)
    and its theta / w; `need` is an int or an [nq] tensor, the number of
    hits a query has to keep. Pure torch, device agnostic.

    For a query with counts > cap the cap retained scores plus the histogram
    of the dropped hits are the whole score distribution above theta:
    H = hist + bins of the retained scores, cum[j] = sum of H[i] for i >= j,
    b* = the lowest j with cum[j] <= cap (the largest candidate set that
    fits), theta2 = edge(b*), expect_n = cum[b*], ok = expect_n >= need. The
    edge and the scan's v > theta2 are the same fp32 comparison, so a rescan
    at theta2 appends exactly expect_n hits. Where even the last bin holds
    more than cap hits nothing fits: theta2 = +inf, expect_n = 0, ok False.

    Queries with counts <= cap are left untouched: theta2 = theta, expect_n
    = counts, ok False (nothing to rescan). Returns (theta2 fp32 [nq],
    expect_n int64 [nq], ok bool [nq])."""
    nq = counts.shape[0]
    over = counts > cap
    b = hist_bin_spec(cand_scores, theta, w)
    H = hist.to(torch.int64).clone()
    H.scatter_add_(1, b, torch.ones_like(b))
    cum = H.flip(1).cumsum(1).flip(1)
    # cum falls with j, so the bins that fit are a suffix
    bstar = HIST_NB - (cum <= cap).sum(dim=1)
    none = bstar == HIST_NB
    cum = torch.cat([cum, cum.new_zeros(nq, 1)], dim=1)
    expect = cum.gather(1, bstar.unsqueeze(1)).squeeze(1)
    theta = theta.float()
    edge = hist_edges(theta, w.float()).gather(1, bstar.unsqueeze(1)).squeeze(1)
    edge = torch.where(none, torch.full_like(edge, float("inf")), edge)
    if not torch.is_tensor(need):
        need = torch.full_like(expect, int(need))
    theta2 = torch.where(over, edge, theta)
    expect_n = torch.where(over, expect, counts.to(torch.int64))
    ok = over & (expect >= need.to(torch.int64))
    return theta2, expect_n, ok


def fp4x4_rescan(Q4, QS, X4, theta2, rows, cap, owner=None, qowner=None, n_swaths=0):
    """Scan the query rows `rows` (int64 [n]) of Q4 / QS again, at
    theta2[rows], with the plain v10 scan (the owned scan with owners).
    Returns (cand_scores, cand_ids, counts) of those n rows. Scan scores
    do not depend on which queries share a block."""
    q4r, qsr = Q4[rows].contiguous(), QS[rows].contiguous()
    th2 = theta2[rows].contiguous()
    if owner is None:
        out = ext().topk_scan_threshold_fp4x4(q4r, qsr, X4[0], X4[1], th2, cap, n_swaths)
    else:
        out = ext().topk_scan_threshold_fp4x4_owned(
            q4r, qsr, X4[0], X4[1], th2, owner, qowner[rows].contiguous(), cap, n_swaths)
    return tuple(out)


def _scan_fp4x4_rescan(Q, Q4, QS, X4, theta, cap, x_norm_bound, owner, qowner, need):
    """The fp4x4 threshold scan with overflow="rescan" (topk_recall_threshold):
    hist scan, plan, rescan of the overflowed queries that the plan can
    place, results scattered back. Returns (cand_scores, cand_ids, counts,
    overflowed, rescanned), the last two as host ints."""
    # bins span theta .. hi; any hi is safe (the last bin is open above).
    # Where that leaves w under a few ulps of the scores (or hi <= theta,
    # or theta = +inf) the bin edges would coincide: a tiny w then puts
    # every hit into the last bin and the query ends at ok = False.
    hi = Q.float().norm(dim=1) * (float(x_norm_bound) * 1.0625)
    w = (hi - theta) / HIST_NB
    floor = torch.maximum(theta.abs(), hi.abs()) * 2.0 ** -20
    w = torch.where(w > floor, w, torch.full_like(w, 1e-30)).contiguous()
    if owner is None:
        cs, ci, counts, hist = ext().topk_scan_threshold_fp4x4_hist(
            Q4, QS, X4[0], X4[1], theta, w, cap, 0)
    else:
        cs, ci, counts, hist = ext().topk_scan_threshold_fp4x4_hist(
            Q4, QS, X4[0], X4[1], theta, w, cap, 0, xowner=owner, qowner=qowner)
    n_over = int((counts > cap).sum())
    if n_over == 0:
        return cs, ci, counts, 0, 0
    theta2, _expect_n, ok = overflow_rescan_plan(cs, counts, hist, theta, w, cap, need)
    rows = ok.nonzero(as_tuple=True)[0]
    n_rows = int(rows.numel())
    if n_rows:
        cs2, ci2, cn2 = fp4x4_rescan(Q4, QS, X4, theta2, rows, cap, owner, qowner)
        cs[rows] = cs2
        ci[rows] = ci2
        counts[rows] = cn2
    return cs, ci, counts, n_over, n_rows


def row_moments(S: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, correction=1 std) of every row of the bf16 GPU matrix S
    [nq, m], fp32 [nq] each, in one pass over S (csrc row_moments_kernel:
    fp64 sums shifted by the row's first element, fixed order). What
    S.float().mean(1) and S.float().std(1) give, up to their own fp32
    reduction error."""
    mu, sigma = ext().row_moments(S.contiguous())
    return mu, sigma


def reference_select_rescore(
    cs: torch.Tensor,
    ci: torch.Tensor,
    counts: torch.Tensor,
    Q: torch.Tensor,
    X: torch.Tensor,
    salience: Optional[torch.Tensor],
    sel: int,
    k: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The recall epilogue in torch, device agnostic: the CPU path, the path
    of the shapes select_rescore's kernel does not take, and the reference
    of its tests. Inputs and outputs as select_rescore."""
    cap = cs.shape[1]
    # mask unfilled/overflowed slots
    slot = torch.arange(cap, device=Q.device).unsqueeze(0)
    valid = slot < counts.clamp_max(cap).unsqueeze(1)
    cs = torch.where(valid, cs, torch.full_like(cs, -1e30))

    # select: top candidates by scan score
    top = torch.topk(cs, sel, dim=1)
    ids = torch.gather(ci, 1, top.indices)

    # exact fp32 rescore of the selected candidates (both dtypes: the
    # bf16 scan's near-ties otherwise reorder the top-k at bf16 precision).
    # salience (membrane semantics) folds into the rescore epilogue:
    # final score = cosine * decayed salience, selection stays by raw
    # cosine with overfetch (salience <= 1 so the weighted top-k is a
    # subset of the higher-cosine candidates in the common case).
    gidx = ids.long().clamp_min(0)
    cand = X[gidx]  # [nq, sel, D]
    exact = torch.einsum("qd,qkd->qk", Q.float(), cand.float())
    if salience is not None:
        exact = exact * salience[gidx]
    exact = torch.where(ids < 0, torch.full_like(exact, -1e30), exact)
    fin = torch.topk(exact, k, dim=1)
    return fin.values, torch.gather(ids, 1, fin.indices)


def select_rescore(
    cs: torch.Tensor,
    ci: torch.Tensor,
    counts: torch.Tensor,
    Q: torch.Tensor,
    X: torch.Tensor,
    salience: Optional[torch.Tensor],
    sel: int,
    k: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Epilogue of the threshold scans: from the candidate buffers cs / ci
    [nq, cap] (fp32 scan scores, int32 row ids; unfilled slots -1e30 / -1)
    and counts [nq] (hits per query, may exceed cap) to the final top-k.
    Of the first min(counts, cap) slots the `sel` best by scan score are
    rescored exactly, dot(Q row, X row) with fp32 sums over the bf16
    values, times salience[id] if given, and the best k of those returned
    as (scores fp32 [nq, k], sorted descending, ids int32 [nq, k]).
    Positions past the valid candidates hold -1e30 / -1.

    On the GPU this is one launch (csrc select_rescore_kernel) for bf16
    Q / X with D % 8 == 0, D <= 2048, k <= sel <= cap <= 1024 and contiguous,
    16-byte aligned tensors; there ties, at the `sel` boundary and in the
    final order, go to the lower row id, so the result is the same from run
    to run whatever order the scan filled the slots in. Every other shape,
    and the CPU, takes reference_select_rescore (torch.topk's tie order)."""
    D = Q.shape[1]
    cap = cs.shape[1]
    native = (
        Q.is_cuda and Q.dtype == torch.bfloat16 and X.dtype == torch.bfloat16
        and D % 8 == 0 and 0 < D <= 2048 and 1 <= k <= sel <= cap <= 1024
        and cs.dtype == torch.float32 and ci.dtype == torch.int32
        and counts.dtype == torch.int32
        and (salience is None or (salience.dtype == torch.float32 and salience.dim() == 1
                                  and salience.is_contiguous()
                                  and salience.numel() >= X.shape[0]))
        and all(t.is_contiguous() for t in (cs, ci, counts, Q, X))
        and Q.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0
    )
    if not native:
        return reference_select_rescore(cs, ci, counts, Q, X, salience, sel, k)
    s, i = ext().select_rescore(cs, ci, counts, Q, X, salience, sel, k)
    return s, i


def topk_recall_threshold(
    Q: torch.Tensor,
    X: torch.Tensor,
    k: int,
    X8: Optional[torch.Tensor] = None,
    sample_rows: int = 131072,
    target_candidates: int = 128,
    cap: int = 1024,
    mx: bool = True,
    X4: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
    q4: bool = True,
    salience: Optional[torch.Tensor] = None,
    owner: Optional[torch.Tensor] = None,
    qowner: Optional[torch.Tensor] = None,
    owner_counts: Optional[torch.Tensor] = None,
    overflow: str = "direct",
    x_norm_bound: float = 1.0,
    stats: Optional[dict] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Threshold-scan recall: per-query score thresholds estimated from a
    sampled pre-pass (Gaussian tail extrapolation), then a fixed-threshold
    scan whose epilogue is just rare global appends — no in-kernel top-k
    maintenance, so the scan runs at its K-loop rate regardless of k.

    With X8 (e4m3 view) the scan runs in fp8 and the top candidates are
    exact-rescored in bf16; final scores are exact either way. `mx` (the
    default, needs D % 128 == 0) runs the fp8 scan on the MX-scaled
    16x16x128 MFMA at unit block scales — same bytes, 2.25x the issue
    rate (csrc topk_scan_mx_kernel). Queries whose candidate buffer
    underflowed (<k survivors: threshold too high for non-Gaussian score
    tails) fall back to the direct kernel.

    `owner` / `qowner` (see topk_recall) filter inside the scan: thresholds
    are set per query from the size of its owner's row set (`owner_counts`
    = cached bincount of `owner`), every candidate is already eligible, and
    the fallback is the owner-filtered direct kernel. Supported by the
    fp4x4 scan (q4, D <= 1024) and the bf16 scan.

    `overflow` is what happens to a query with more than `cap` hits above
    its threshold (clustered content: the Gaussian tail does not describe
    it). "direct" sends it to the direct kernel over the whole index.
    "rescan" (fp4x4 scan only: q4, D <= 1024, with or without owners) has
    the scan count the hits it drops in a 256-bin score histogram per query
    (csrc topk_scan_fp4_hist_kernel; bins span theta .. |q| * x_norm_bound *
    1.0625, scores past that land in the open last bin), picks from it the
    lowest bin edge above which at most `cap` hits lie
    (overflow_rescan_plan) and rescans only those queries at that threshold,
    which then fits exactly. `x_norm_bound` bounds the row norms of X. A
    query whose top `cap` hits sit inside one bin with fewer than k above it
    still goes to the direct kernel, as underflowed queries do.

    `stats`, if a dict, receives the number of queries that `overflowed`,
    were `rescanned` and took the `direct_fallback`, in both modes.
    """
    if overflow not in ("direct", "rescan"):
        raise ValueError(f"overflow must be 'direct' or 'rescan', not {overflow!r}")
    nq, D = Q.shape
    nx = X.shape[0]
    m = min(nx, sample_rows)
    use_fp4 = X4 is not None and D % 128 == 0 and D <= 2048
    use_fp8 = X8 is not None or use_fp4
    use_mx = mx and X8 is not None and D % 128 == 0
    owner, qowner = _owner_args(owner, qowner)
    if owner is not None and use_fp8 and not (use_fp4 and q4 and D <= 1024):
        raise NotImplementedError(
            "owner-filtered recall: fp4x4 (q4, D <= 1024) and bf16 scans only")
    rescan = overflow == "rescan"
    if rescan and not (use_fp4 and q4 and D <= 1024):
        raise NotImplementedError(
            "overflow='rescan': fp4x4 scan (q4, D <= 1024) only")

    # 1. per-query score statistics from a sample (bf16 matmul); on the GPU
    # both moments come from one pass over the bf16 scores (row_moments)
    sample = torch.matmul(Q, X[:m].T)  # [nq, m]
    if sample.is_cuda and sample.dtype == torch.bfloat16 and m >= 2:
        mu, sigma = row_moments(sample)
    else:
        sample = sample.float()
        mu = sample.mean(dim=1)
        sigma = sample.std(dim=1)
    sigma = sigma.clamp_min(1e-6)
    # Gaussian tail: P(score > theta) = C/nx
    p = min(0.5, max(target_candidates / max(nx, 1), 1e-12))
    try:
        from scipy.stats import norm

        z = float(norm.ppf(1.0 - p))
    except ImportError:  # pragma: no cover
        import math

        # Beasley-Springer-Moro style rough inverse via bisection
        lo, hi = 0.0, 9.0
        for _ in range(60):
            mid = (lo + hi) / 2
            if 0.5 * math.erfc(mid / math.sqrt(2)) > p:
                lo = mid
            else:
                hi = mid
        z = (lo + hi) / 2
    # fp4 scan scores carry quantization noise (~0.2 sigma): lower theta
    # so near-threshold true candidates still land in the buffer, and
    # widen the rescore window below (select is by NOISY scan score).
    if use_fp4:
        z = z - 0.25
    if owner is None:
        theta = (mu + sigma * z).contiguous()
    else:
        if owner_counts is None:
            owner_counts = torch.bincount(owner.long())
        n_all = torch.full((1,), nx, dtype=owner_counts.dtype, device=Q.device)
        # a query owner past the table owns no row
        cnt = torch.cat([owner_counts.to(Q.device), n_all.new_zeros(1)])
        qo = qowner.long()
        n_owned = torch.where(
            qo < 0, n_all.expand(nq),
            cnt[qo.clamp(0, cnt.numel() - 1)])
        theta = owned_thresholds(
            mu, sigma, n_owned, target_candidates,
            z_margin=0.25 if use_fp4 else 0.0).contiguous()

    # 2. fixed-threshold scan
    if use_fp4 and q4 and D <= 1024:
        # both operands MXFP4: scores carry no static prescale
        # (one fused launch, bit-exact with to_fp4_mx)
        Q4, QS = quantize_fp4_mx(Q)
        if rescan:
            cs, ci, counts, n_over, n_rescanned = _scan_fp4x4_rescan(
                Q, Q4, QS, X4, theta, cap, x_norm_bound, owner, qowner,
                k if owner is None else n_owned.clamp_max(k))
        elif owner is None:
            cs, ci, counts = ext().topk_scan_threshold_fp4x4(
                Q4, QS, X4[0], X4[1], theta.contiguous(), cap, 0)
        else:
            cs, ci, counts = ext().topk_scan_threshold_fp4x4_owned(
                Q4, QS, X4[0], X4[1], theta, owner, qowner, cap, 0)
    elif use_fp4:
        # Q carries the only static scale (x8); X scales are per-block
        Q8 = to_fp8_bytes(Q)
        cs, ci, counts = ext().topk_scan_threshold_fp4(
            Q8, X4[0], X4[1], (theta * 8.0).contiguous(), cap, 0)
    elif use_fp8:
        Q8 = to_fp8_bytes(Q)
        # thresholds are in fp8-score units: inputs scaled x8 each -> x64
        cs, ci, counts = ext().topk_scan_threshold(Q8, X8, (theta * 64.0).contiguous(),
                                                   cap, 0, True, use_mx)
    elif owner is None:
        cs, ci, counts = ext().topk_scan_threshold(Q, X, theta, cap, 0, False, False)
    else:
        cs, ci, counts = ext().topk_scan_threshold(
            Q, X, theta, cap, 0, False, False, xowner=owner, qowner=qowner)

    # 3.-4. select the top candidates by scan score (wider for the noisier
    # fp4 scan, and for salience weighting — the weighted top-k can sit
    # below the raw-cosine top-2k; the exact rescore makes overfetch
    # nearly free), rescore them exactly and keep the top k
    if use_fp4 or salience is not None:
        sel = min(cap, max(8 * k if salience is not None else 4 * k, 128))
    else:
        sel = min(cap, max(2 * k, 32))
    out_s, out_i = select_rescore(cs, ci, counts, Q, X, salience, sel, k)

    # 5. fallback for underflowed queries (non-Gaussian tails / theta high)
    if owner is None:
        bad = (counts < k) | (counts > cap)
    else:
        # an owner with fewer than k rows legitimately underfills: those
        # queries are done once every owned row is a candidate
        bad = (counts < n_owned.clamp_max(k)) | (counts > cap)
    if stats is None:
        any_bad = bool(bad.any())
    else:
        # one host read for both figures
        n_of, n_bad = torch.stack([(counts > cap).sum(), bad.sum()]).tolist()
        stats["overflowed"] = n_over if rescan else n_of
        stats["rescanned"] = n_rescanned if rescan else 0
        stats["direct_fallback"] = n_bad
        any_bad = n_bad > 0
    if any_bad:
        rows = bad.nonzero(as_tuple=True)[0]
        k2f = min(4 * k, 32, X.shape[0])  # the direct kernel's k bound
        if owner is None:
            fb_s, fb_i = topk_recall(Q[rows].contiguous(), X, k2f)
        else:
            fb_s, fb_i = topk_recall(Q[rows].contiguous(), X, k2f, owner=owner,
                                     qowner=qowner[rows].contiguous())
        # exact fp32 rescore (+ salience weight) so fallback rows report
        # the same score definition as the main path
        fb_g = fb_i.long().clamp_min(0)
        fb_exact = torch.einsum("qd,qkd->qk", Q[rows].float(), X[fb_g].float())
        if salience is not None:
            fb_exact = fb_exact * salience[fb_g]
        fb_exact = torch.where(fb_i < 0, torch.full_like(fb_exact, -1e30), fb_exact)
        ft = torch.topk(fb_exact, k, dim=1)
        out_s[rows] = ft.values
        out_i[rows] = torch.gather(fb_i, 1, ft.indices)
    return out_s, out_i


def topk_recall_threshold_banded(
    Q: torch.Tensor,
    X: torch.Tensor,
    k: int,
    salience: torch.Tensor,
    hot_idx: torch.Tensor,
    hot_X: Optional[torch.Tensor] = None,
    is_hot: Optional[torch.Tensor] = None,
    **kw,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Salience-banded weighted recall for SKEWED salience distributions.

    The bounded-overfetch weighted path (topk_recall_threshold with
    salience) selects by raw cosine; under heavy skew (e.g. Zipf with a
    100x range) the dense weighted optimum can sit at cosine rank ~10k —
    beyond any bounded overfetch (measured ~86% dense-regret at 128
    candidates; the reference's interactive limit*4 overfetch has the
    same bound, membrane retrieve path). This variant recovers those
    optima: the HOT band (top-salience rows, `hot_idx`) is scored
    exactly — dense weighted bf16 matmul over a small gathered copy — so
    no cosine-rank bound applies there, while the COLD band keeps the
    fp4 threshold scan. Bands merge by exact weighted score; cold
    candidates that are hot rows are masked out (the hot band already
    scored them exactly), so no duplicates survive.

    `hot_X` (gathered rows) and `is_hot` (membership mask) are optional
    caches the caller refreshes when salience order drifts.
    """
    nh = int(hot_idx.numel())
    if nh == 0:
        return topk_recall_threshold(Q, X, k, salience=salience, **kw)
    if hot_X is None:
        hot_X = X[hot_idx.long()]
    hot = torch.matmul(Q, hot_X.T).float() * salience[hot_idx.long()]
    owner, qowner = _owner_args(kw.get("owner"), kw.get("qowner"))
    if owner is not None:
        # hot band under the owner filter: foreign rows never reach its top-k
        qo = qowner.long().unsqueeze(1)
        eligible = (qo < 0) | (owner[hot_idx.long()].long().unsqueeze(0) == qo)
        hot = torch.where(eligible, hot, torch.full_like(hot, -1e30))
    hs, hsel = torch.topk(hot, min(k, nh), dim=1)
    hi = hot_idx[hsel.reshape(-1)].reshape(hsel.shape).to(torch.int32)
    if owner is not None:
        hi = torch.where(hs > -1e29, hi, torch.full_like(hi, -1))

    cs, ci = topk_recall_threshold(Q, X, k, salience=salience, **kw)
    if is_hot is None:
        is_hot = torch.zeros(X.shape[0], dtype=torch.bool, device=X.device)
        is_hot[hot_idx.long()] = True
    dup = is_hot[ci.long().clamp_min(0)]
    cs = torch.where(dup, torch.full_like(cs, -1e30), cs)
    if owner is not None:
        # an owner short of k rows fills its tail from masked slots: they
        # must not carry the id of a row the hot band already returned
        ci = torch.where(dup, torch.full_like(ci, -1), ci)

    all_s = torch.cat([hs, cs], dim=1)
    all_i = torch.cat([hi, ci], dim=1)
    fin = torch.topk(all_s, k, dim=1)
    return fin.values, torch.gather(all_i, 1, fin.indices)


# -- fact-registry probe ----------------------------------------------------

FNV_OFFSET = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
_U64 = (1 << 64) - 1

# claim bit -> canonical predicate, per the reference's claim-type ->
# predicate strategy table (fact-checker.ts:127-136) over the CLAIMS
# family bits (ops/pattern_sets.py CLAIMS_PATTERNS). Types whose
# strategy is NOT a single predicate (entity_name matches by subject
# alone; self_referential matches the "self" subject) have no entry —
# the GPU probe skips those bits and the host FactRegistry path covers
# them.
CLAIM_BIT_PREDICATE: Dict[int, str] = {
    0: "state",       # system_state -> "state"
    2: "exists",      # existence_pos
    3: "exists",      # existence_neg
    4: "exists",      # there_is
    5: "metric",      # has/contains/uses numeric
    6: "percentage",  # percentage
    7: "count",       # count
}


def fnv1a64(data: bytes) -> int:
    h = FNV_OFFSET
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & _U64
    return h


def _mix_key(subject_h: int, predicate_h: int) -> int:
    """Continues the subject FNV stream through '|' + predicate-hash bytes
    (bit-exact with csrc/fact_probe.hip mix_key)."""
    h = ((subject_h ^ ord("|")) * FNV_PRIME) & _U64
    for i in range(8):
        h = ((h ^ ((predicate_h >> (8 * i)) & 0xFF)) * FNV_PRIME) & _U64
    return h


def _tokenize_fact(data: bytes) -> list:
    """Word tokens (>=2 chars, lowercased) under the probe kernel's
    byte classes: [a-z0-9_.-]."""
    toks = []
    cur = bytearray()
    for b in data + b" ":
        c = bytes([b]).lower()[0]
        if (48 <= c <= 57) or (97 <= c <= 122) or c in (95, 45, 46):
            cur.append(c)
        elif cur:
            if len(cur) >= 2:
                toks.append(bytes(cur))
            cur = bytearray()
    return toks


def build_fact_table(facts: Sequence[Tuple[str, str, str]], pow2: Optional[int] = None):
    """Pack (subject, predicate, object) triples into the open-addressing
    probe table: keys/vals int64 tensors + the per-claim-bit predicate
    hash vector. Single-token subjects/objects only (multi-word facts stay
    on the host FactRegistry path — see csrc/fact_probe.hip header)."""
    if pow2 is None:
        pow2 = max(4, (len(facts) * 2 - 1).bit_length())
    size = 1 << pow2
    keys = np.zeros(size, dtype=np.uint64)
    vals = np.zeros(size, dtype=np.uint64)
    for subject, predicate, obj in facts:
        sh = fnv1a64(subject.strip().lower().encode())
        ph = fnv1a64(predicate.strip().lower().encode())
        key = _mix_key(sh, ph) or 1
        slot = key & (size - 1)
        for _ in range(size):
            if keys[slot] == 0 or keys[slot] == key:
                break
            slot = (slot + 1) % size
        keys[slot] = key
        vals[slot] = fnv1a64(obj.strip().lower().encode())
    pred = np.zeros(64, dtype=np.uint64)
    for bit, p in CLAIM_BIT_PREDICATE.items():
        pred[bit] = fnv1a64(p.encode())
    return (
        torch.from_numpy(keys.view(np.int64)),
        torch.from_numpy(vals.view(np.int64)),
        torch.from_numpy(pred.view(np.int64)),
        pow2,
    )


def fact_probe(
    bytes_t: torch.Tensor,
    offsets: torch.Tensor,
    claims_mask: torch.Tensor,
    table_keys: torch.Tensor,
    table_vals: torch.Tensor,
    pred_hash: torch.Tensor,
    pow2: int,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-message (verified, contradicted) counts (csrc/fact_probe.hip)."""
    v, c = ext().fact_probe(bytes_t, offsets, claims_mask, pred_hash,
                            table_keys, table_vals, pow2)
    return v, c


def reference_fact_probe(
    messages: Sequence[bytes], claims_masks: Sequence[int],
    facts: Sequence[Tuple[str, str, str]],
) -> Tuple[np.ndarray, np.ndarray]:
    """CPU mirror of the probe kernel's semantics for the numerics tests."""
    table = {}
    for subject, predicate, obj in facts:
        key = _mix_key(fnv1a64(subject.strip().lower().encode()),
                       fnv1a64(predicate.strip().lower().encode())) or 1
        table[key] = fnv1a64(obj.strip().lower().encode())
    ver = np.zeros(len(messages), dtype=np.int32)
    con = np.zeros(len(messages), dtype=np.int32)
    for i, (msg, cmask) in enumerate(zip(messages, claims_masks)):
        if not cmask:
            continue
        toks = [fnv1a64(t) for t in _tokenize_fact(msg)][:96]
        for bit, predicate in CLAIM_BIT_PREDICATE.items():
            if not (cmask >> bit) & 1:
                continue
            ph = fnv1a64(predicate.encode())
            for t in toks:
                key = _mix_key(t, ph) or 1
                val = table.get(key)
                if val is None:
                    continue
                if val in toks:
                    ver[i] += 1
                else:
                    con[i] += 1
    return ver, con


# -- batched envelopes + all-family scan ------------------------------------

def build_envelopes(records_cpu: torch.Tensor, session: str,
                    agent_prefix: str = "agent",
                    ctype: str = "message.in.received") -> bytes:
    """One ClawEvent JSONL line per audit record (csrc/host_envelope.cpp,
    GIL released). Line format parity with eventstore.hooks.build_envelope
    is covered by tests/test_eventstore.py."""
    return ext().build_envelopes(records_cpu, session, agent_prefix, ctype)


class DeviceFamilySet:
    """All families' packed tables concatenated for the one-launch scan
    (csrc dfa_scan_multi_kernel): per-family (begin, end) sub-DFA ranges
    into the shared meta table."""

    def __init__(self, names: Sequence[str], device) -> None:
        import numpy as _np

        self.names = list(names)
        nexts, accepts, eofs, cmaps, metas, ranges = [], [], [], [], [], []
        state_base = 0
        next_base = 0
        row = 0
        for name in self.names:
            packed = pattern_sets.get_family(name).pack()
            meta = packed["meta"].copy()
            n_dfas = meta.shape[0]
            meta[:, 0] += next_base
            meta[:, 1] += state_base
            meta[:, 3] += row
            ranges.append((row, row + n_dfas))
            row += n_dfas
            next_base += packed["next"].size
            state_base += packed["accept"].size
            nexts.append(packed["next"])
            accepts.append(packed["accept"])
            eofs.append(packed["eof"])
            cmaps.append(packed["class_maps"])
            metas.append(meta)
        self.next = torch.from_numpy(_np.concatenate(nexts).view(_np.int16)).to(device)
        self.accept = torch.from_numpy(_np.concatenate(accepts).view(_np.int64)).to(device)
        self.eof = torch.from_numpy(_np.concatenate(eofs).view(_np.int64)).to(device)
        self.class_maps = torch.from_numpy(
            _np.concatenate(cmaps).reshape(-1)
        ).to(device)
        self.meta = torch.from_numpy(_np.concatenate(metas)).to(device)
        self.ranges = torch.from_numpy(
            _np.array(ranges, dtype=_np.int32)
        ).to(device)


_device_family_sets: Dict[Tuple[Tuple[str, ...], int], DeviceFamilySet] = {}


def device_family_set(names: Sequence[str], device) -> DeviceFamilySet:
    dev = torch.device(device)
    key = (tuple(names), dev.index if dev.index is not None else -1)
    if key not in _device_family_sets:
        _device_family_sets[key] = DeviceFamilySet(names, dev)
    return _device_family_sets[key]


def dfa_scan_all(bytes_t: torch.Tensor, offsets: torch.Tensor,
                 families: Sequence[str]) -> Dict[str, torch.Tensor]:
    """All families in ONE kernel launch; returns {family: hit masks}."""
    fs = device_family_set(families, bytes_t.device)
    hits = ext().dfa_scan_multi(bytes_t, offsets, fs.next, fs.accept, fs.eof,
                                fs.class_maps, fs.meta, fs.ranges)
    return {name: hits[i] for i, name in enumerate(fs.names)}
