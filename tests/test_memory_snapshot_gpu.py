"""Snapshot and restore of the live memory: a fresh pipeline that loads a
snapshot holds the saver's rows bit for bit (the MXFP4 copy requantized),
goes on exactly as the saver does, hands out new ids, and refuses
snapshots that do not fit without touching its state."""

import json
import os

import numpy as np
import pytest
import torch

from vainplex_openclaw_amd.pipeline.engine import V_DENY, FirewallPipeline, PipelineConfig
from vainplex_openclaw_amd.pipeline.synth import TOOL_RISKS, SynthBatch, synthetic_conversations

pytestmark = pytest.mark.gpu

BASE = dict(batch=256, dim=256, vocab=4096, index_size=2048, topk=8)
N0, SPARE = 2048, 600
STEP_KEYS = ("verdict", "risk", "recall_scores", "recall_ids", "recall_mem_ids",
             "memory_ids", "trust_scores")


def _cfg(**kw):
    base = dict(BASE)
    for k in ("dim", "index_size"):
        if k in kw:
            base[k] = kw.pop(k)
    kw.setdefault("recall_isolation", True)
    return PipelineConfig(**base, recall_mode="threshold", memory_ids=True, ingest=True,
                          ingest_capacity=kw.pop("spare", SPARE), ingest_full="evict", **kw)


def make_batch(seed):
    """240 distinct random-letter messages (no two rows tie) and 16 synthetic
    conversation messages, injections and credentials among them."""
    rng = np.random.default_rng(seed)
    msgs = [rng.integers(97, 123, size=300, dtype=np.uint8).tobytes() for _ in range(240)]
    agents = rng.integers(0, 64, size=240).astype(np.int32)
    risks = rng.choice(TOOL_RISKS, size=240).astype(np.float32)
    conv = synthetic_conversations(256, seed=seed)
    pick = list(np.nonzero(conv.labels == 1)[0][:6]) + list(np.nonzero(conv.labels == 2)[0][:4])
    pick += list(np.nonzero(conv.labels == 0)[0][:16 - len(pick)])
    assert len(pick) == 16
    msgs += [conv.messages[i] for i in pick]
    assert len(set(msgs)) == len(msgs), "identical messages would tie in recall"
    return SynthBatch(msgs, np.concatenate([agents, conv.agent_idx[pick]]),
                      np.concatenate([risks, conv.tool_risk[pick]]),
                      np.concatenate([np.zeros(240, dtype=np.int8), conv.labels[pick]]))


def _state(pipe):
    """The state vectors a snapshot carries, live rows only, as bit patterns."""
    n = pipe.n_rows
    st = {
        "n_rows": n,
        "messages_seen": pipe.messages_seen,
        "index": pipe.index[:n].view(torch.int16).clone(),
        "codes": pipe.index4[0][:n].clone(),
        "scales": pipe.index4[1][:n].clone(),
        "salience": pipe.salience[:n].view(torch.int32).clone(),
        "index_ids": pipe.index_ids[:n].clone(),
        "trust": torch.stack([v for _k, v in sorted(pipe.trust_state.items())]).view(torch.int32),
        "cortex": torch.cat([v for _k, v in sorted(pipe.cortex_state.items())]),
    }
    if pipe.index_owner is not None:
        st["index_owner"] = pipe.index_owner[:n].clone()
        st["owner_counts"] = pipe.owner_counts.clone()
    return st


def _assert_same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], int):
            assert a[k] == b[k], k
        else:
            assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """Pipeline A after three steps (an eviction among them) and its
    snapshot, written in several chunks with a ragged last one."""
    a = FirewallPipeline(_cfg(), device="cuda:0")
    handed = []
    for seed in (201, 202, 203):
        out = a.step(make_batch(seed))
        keep = out["verdict"] != V_DENY
        assert 200 < int(keep.sum()) < BASE["batch"]
        handed.append(out["memory_ids"][keep])
    assert a.forgotten > 0, "the third step must overrun the spare rows"
    assert a.n_rows % 1000 != 0 and a.n_rows > 2000
    path = str(tmp_path_factory.mktemp("snap") / "rank0")
    man = a.save_memory(path, chunk_rows=1000)
    assert man["counters"]["forgotten"] == a.forgotten
    assert man["counters"]["forget_epoch"] == a.forget_epoch > 0
    return a, path, man, _state(a), torch.cat(handed)


def test_snapshot_files(saved):
    _a, path, man, st, _handed = saved
    n = st["n_rows"]
    with open(os.path.join(path, "manifest.json")) as f:
        assert json.load(f) == man
    assert man["format"] == 1 and man["dim"] == 256 and man["n_rows"] == n
    assert man["rank"] == 0 and man["world_size"] == 1
    assert man["columns"] == {"owner": True, "ids": True}
    want = {"index.bf16": n * 256 * 2, "salience.f32": n * 4, "owner.i32": n * 4,
            "ids.i64": n * 8}
    for name, size in want.items():
        assert os.path.getsize(os.path.join(path, name)) == size == man["files"][name]
    assert sorted(os.listdir(path)) == sorted(list(want) + ["manifest.json", "state.npz"])
    assert not [d for d in os.listdir(os.path.dirname(path)) if ".tmp-" in d]
    c = man["counters"]
    assert c["messages_seen"] == 3 * 256 and c["batch_seq"] == 3 and c["_steps_done"] == 3
    assert c["ingest_dropped"] == 0 and c["recall_overflowed"] == 0
    # the live prefix, raw little-endian
    ids = np.fromfile(os.path.join(path, "ids.i64"), dtype="<i8")
    assert np.array_equal(ids, st["index_ids"].cpu().numpy())
    rows = np.fromfile(os.path.join(path, "index.bf16"), dtype="<i2").reshape(n, 256)
    assert np.array_equal(rows, st["index"].cpu().numpy())


def test_resume_equivalence(saved):
    a, path, man, st_a, handed = saved
    assert _state(a)["messages_seen"] == st_a["messages_seen"], "A must not have moved on"
    b = FirewallPipeline(_cfg(), device="cuda:0")
    b.load_memory(path)
    _assert_same_state(st_a, _state(b))
    assert b.forget_epoch == man["counters"]["forget_epoch"] + 1
    for k in ("batch_seq", "_steps_done", "forgotten", "ingest_dropped", "recall_overflowed",
              "recall_rescanned", "recall_direct_fallbacks"):
        assert getattr(b, k) == getattr(a, k), k
    new_ids = []
    for seed in (204, 205):
        batch = make_batch(seed)
        out_a = a.step(batch)
        out_b = b.step(batch)
        for k in STEP_KEYS:
            assert out_a[k].dtype == out_b[k].dtype
            assert torch.equal(out_a[k].view(torch.uint8), out_b[k].view(torch.uint8)), k
        _assert_same_state(_state(a), _state(b))
        new_ids.append(out_b["memory_ids"])
    assert a.recall_overflowed == 0 and b.recall_overflowed == 0
    # ids do not restart: what B hands out is in no way in the snapshot
    new_ids = torch.cat(new_ids)
    new_ids = new_ids[new_ids >= 0]
    assert new_ids.numel() > 400
    assert not torch.isin(new_ids, st_a["index_ids"]).any()
    assert not torch.isin(new_ids, handed).any()
    assert int(new_ids.min()) >= 3 * 256


def test_load_replaces_whatever_was_there(saved):
    """Loading into a pipeline that has run, and has more capacity."""
    _a, path, man, st_a, _handed = saved
    b = FirewallPipeline(_cfg(spare=SPARE + 333), device="cuda:0")
    b.step(make_batch(301))
    for _ in range(3):
        assert b.forget(count=10) == 10
    assert b.forget_epoch == 3 > man["counters"]["forget_epoch"]
    b.load_memory(path)
    _assert_same_state(st_a, _state(b))
    assert b.forget_epoch == 4
    assert b.capacity == N0 + SPARE + 333


def test_save_refuses_existing_path(saved, tmp_path):
    a, path, _man, _st, _handed = saved
    with pytest.raises(ValueError):
        a.save_memory(path)
    other = tmp_path / "there"
    other.mkdir()
    with pytest.raises(ValueError):
        a.save_memory(str(other))
    assert os.listdir(other) == []


def _truncated_copy(path, tmp_path):
    import shutil

    bad = str(tmp_path / "truncated")
    shutil.copytree(path, bad)
    rows = os.path.join(bad, "index.bf16")
    with open(rows, "r+b") as f:
        f.truncate(os.path.getsize(rows) - 512)
    return bad


@pytest.mark.parametrize("case", ["dim", "capacity", "isolation", "seed", "truncated"])
def test_load_refusals_leave_state_untouched(saved, tmp_path, case):
    _a, path, _man, _st, _handed = saved
    cfg = {
        "dim": lambda: _cfg(dim=128),
        "capacity": lambda: _cfg(index_size=1024),
        "isolation": lambda: _cfg(recall_isolation=False),
        "seed": lambda: _cfg(seed=77),
        "truncated": lambda: _cfg(),
    }[case]()
    b = FirewallPipeline(cfg, device="cuda:0")
    b.step(make_batch(401))
    before = _state(b)
    counters = {k: getattr(b, k) for k in ("forget_epoch", "batch_seq", "_steps_done")}
    src = _truncated_copy(path, tmp_path) if case == "truncated" else path
    with pytest.raises(ValueError):
        b.load_memory(src)
    _assert_same_state(before, _state(b))
    assert counters == {k: getattr(b, k) for k in counters}
