"""CPU: bench.py's pieces outside the timed steps -- the replayed input batches (later_batch) and
the output dump (dump_outputs) -- over a stand-in context that serves host arrays."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from easydarwin_amd import edgpu  # noqa: E402


def test_later_batch_moves_only_the_arrival_times():
    desc = np.zeros(5, dtype=edgpu.PKT_DTYPE)
    desc["slot"] = np.arange(5) * 7
    desc["len"] = 1400 - np.arange(5)
    desc["channel"] = [0, 0, 1, 0, 0]
    desc["flags"] = 3
    desc["arrival_ms"] = [0, 5, 999, -4, 2**40]
    bt = {"desc": torch.from_numpy(desc.view(np.uint8).copy()), "t": 1000, "n": 5, "bytes": 7000,
          "blob": torch.zeros(16, dtype=torch.uint8)}
    nb = bench.later_batch(None, bt, 3000)
    got = nb["desc"].numpy().view(edgpu.PKT_DTYPE)
    assert nb["t"] == 4000 and nb["blob"] is bt["blob"] and nb["n"] == 5
    for k in ("slot", "len", "channel", "flags"):
        assert (got[k] == desc[k]).all()
    assert (got["arrival_ms"] == desc["arrival_ms"] + 3000).all()
    assert (bt["desc"].numpy().view(edgpu.PKT_DTYPE)["arrival_ms"] == desc["arrival_ms"]).all()   # the resident one stays
    reads = np.zeros(3, dtype=edgpu.TCP_READ_DTYPE)
    reads["arrival_ms"] = [1, 2, 3]
    nt = bench.later_batch(None, {"tcp": {"reads": reads, "raw": None, "raw_bytes": 9}, "t": 10}, 50)
    assert nt["tcp"]["reads"]["arrival_ms"].tolist() == [51, 52, 53] and reads["arrival_ms"].tolist() == [1, 2, 3]


class _HostCtx:
    """copy_to_host / stats over host memory: 'device pointers' are offsets into one buffer."""

    def __init__(self, mem, st):
        self.mem, self.st = mem, st

    def stats(self):
        return self.st

    def copy_to_host(self, ptr, nbytes):
        return self.mem[int(ptr):int(ptr) + int(nbytes)].copy()


def _fake_tick(npk=5000, nsub=40, seed=1):
    rng = np.random.default_rng(seed)
    ln = rng.integers(12, 1461, npk).astype(np.uint32)
    desc = np.zeros(npk, dtype=edgpu.OUT_DTYPE)
    desc["len"] = ln
    desc["offset"] = np.concatenate([[0], np.cumsum((ln + 15) // 16 * 16)[:-1]])
    desc["packet_id"] = rng.integers(0, 2**32, npk)
    arena = rng.integers(0, 256, int(desc["offset"][-1]) + int(ln[-1]), dtype=np.uint8)
    subs = np.zeros(nsub, dtype=edgpu.SUB_DTYPE)
    subs["subscriber"] = np.arange(nsub)
    subs["desc_count"] = npk // nsub
    subs["desc_base"] = np.arange(nsub) * (npk // nsub)
    a0 = 64
    s0 = a0 + arena.nbytes
    d0 = s0 + subs.nbytes
    mem = np.concatenate([np.zeros(a0, np.uint8), arena, subs.view(np.uint8), desc.view(np.uint8)])
    st = types.SimpleNamespace(relayed_packets=npk, relayed_bytes=int(ln.sum()), arena_bytes=arena.nbytes,
                               pass_packets=npk, pass_arena_bytes=arena.nbytes, status=0)
    r = types.SimpleNamespace(arena=a0, desc=d0, substreams=s0, n_substreams=nsub)
    return _HostCtx(mem, st), r, desc, arena, subs


def test_dump_outputs_is_a_fixed_sample_of_what_the_fanout_returned(tmp_path):
    ctx, r, desc, arena, subs = _fake_tick()
    info = bench.dump_outputs(ctx, r, str(tmp_path / "a"))
    bench.dump_outputs(ctx, r, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in info["arrays"]) and info["bytes"] <= 64 << 20
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:                                           # the same tick gives the same files
        again = np.load(tmp_path / "b" / f)
        assert again.dtype == got[f[:-4]].dtype and np.array_equal(again, got[f[:-4]])
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) == info["bytes"]
    assert got["tick_stats"].tolist() == [5000, int(desc["len"].sum()), arena.nbytes, 5000, arena.nbytes, 40, 0]
    assert got["desc_totals"].tolist() == [5000, float(desc["len"].sum()), float(desc["offset"].sum()),
                                           float(desc["packet_id"].sum(dtype=np.float64))]
    assert (got["substreams"][:, 0] == np.arange(40)).all() and (got["substreams"][:, 6] == subs["desc_count"]).all()
    idx = got["desc_sample"][:, 0].astype(np.int64)
    assert len(idx) == 5000 and (np.diff(idx) > 0).all()
    assert (got["desc_sample"][:, 1] == desc["offset"][idx]).all() and (got["desc_sample"][:, 2] == desc["len"][idx]).all()
    pk = got["packet_index"].astype(np.int64)
    assert len(pk) == len(got["packet_bytes"]) > 0
    for row, k in zip(got["packet_bytes"], pk):               # whole packets, byte for byte, padded with -1
        off, ln = int(desc["offset"][k]), int(desc["len"][k])
        assert (row[:ln] == arena[off:off + ln]).all() and (row[ln:] == -1).all()
    # another tick's bytes show in the dump
    ctx.mem[r.arena + int(desc["offset"][pk[0]])] ^= 0xFF
    bench.dump_outputs(ctx, r, str(tmp_path / "c"))
    assert not np.array_equal(np.load(tmp_path / "c" / "packet_bytes.npy"), got["packet_bytes"])
