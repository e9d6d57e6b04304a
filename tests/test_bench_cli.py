"""bench.py command line: --dump-outputs and --full.

The dump is what lets two builds be compared output for output, so the
contract checked here is: float32/float64 .npy files only, integers
stored exactly (64-bit hit masks as two 32-bit halves), under the 64 MB
cap, and identical between two runs with the same arguments.
"""

import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_exact_float_arrays(tmp_path):
    mask = torch.tensor([0, 1, (1 << 63) - 1, -1, 0x1234_5678_9ABC_DEF0], dtype=torch.int64)
    out = {
        "verdict": torch.tensor([0, 2, 1], dtype=torch.int32),
        "features": torch.tensor([[0.5, -1.25]], dtype=torch.bfloat16),
        "recall_ids": torch.tensor([[49_999_999, -1]], dtype=torch.int32),
        "hits": {"injection": mask},
        "merkle_root": torch.zeros(32, dtype=torch.uint8),
        "cortex": {"decisions": torch.tensor([3, 0], dtype=torch.int64)},
    }
    d = str(tmp_path / "dump")
    bench.dump_outputs(out, d)
    got = _load_dir(d)
    assert set(got) == {"verdict", "features", "recall_ids", "hits_injection_lo",
                        "hits_injection_hi", "cortex_decisions"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["features"].dtype == np.float32
    assert got["features"].tolist() == [[0.5, -1.25]]
    assert got["recall_ids"].tolist() == [[49_999_999.0, -1.0]]
    assert got["cortex_decisions"].tolist() == [3.0, 0.0]
    # the two halves reassemble every 64-bit mask exactly
    lo = got["hits_injection_lo"].astype(np.uint64)
    hi = got["hits_injection_hi"].astype(np.uint64)
    assert ((hi << np.uint64(32)) | lo).tolist() == mask.numpy().view(np.uint64).tolist()


def test_dump_outputs_refuses_more_than_64mb(tmp_path):
    big = {"features": torch.zeros(17 << 20, dtype=torch.float32)}  # 68 MB
    with pytest.raises(RuntimeError, match="64 MB"):
        bench.dump_outputs(big, str(tmp_path / "dump"))


def _run_bench(monkeypatch, capsys, extra):
    argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
            "--batch", "256", "--index", "131072", "--topk", "8"] + extra
    monkeypatch.setattr(sys, "argv", argv)
    assert bench.main() == 0
    cap = capsys.readouterr()
    lines = [ln for ln in cap.out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), cap.err


@pytest.mark.gpu
def test_bench_dump_is_reproducible_and_full_is_opt_in(tmp_path, monkeypatch, capsys):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    res, err = _run_bench(monkeypatch, capsys, ["--dump-outputs", d1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["unit"] == "msg/s" and res["higher_is_better"] is True
    # a plain run prints nothing beyond its result line
    assert "journal_events_replayed" not in err and "stage ms/step" not in err

    res2, err2 = _run_bench(monkeypatch, capsys, ["--dump-outputs", d2, "--full"])
    assert "stage ms/step" in err2
    acct = json.loads([ln for ln in err2.splitlines() if "journal_events_replayed" in ln][0])
    # warmup + timed + the 3 instrumented stage-timing steps, 256 messages each
    assert acct["journal_events_replayed"] == acct["journal_expected"] == (1 + 2 + 3) * 256
    assert acct["journal_events_timed"] == 2 * 256

    a, b = _load_dir(d1), _load_dir(d2)
    assert set(a) == set(b) and "merkle_root" not in a
    for name in ("verdict", "risk", "logits", "features", "recall_scores", "recall_ids",
                 "trust_scores", "validation", "hits_injection_lo", "cortex_decisions"):
        assert name in a
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["recall_ids"].shape == (256, 8) and a["features"].shape == (256, 1024)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert np.array_equal(a[name], b[name]), name
