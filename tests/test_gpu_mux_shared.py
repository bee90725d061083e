"""GPU: the three muxes of tapped units on one context.  They share their staging (the ES copy, the
output staging, the units copy, the start-code bitmap, chunk table and distance table) and, in
Context, one device ES buffer, so calls of different formats are interleaved here, a small input
after a large one (stale bitmap and distance words, stale staging bytes), and every call is held
against its format's CPU model: tests/ts_model.py, mp4_model.py, flv_model.py.

The large input spans two 2-KiB start-code chunks (2 KiB + 40 bytes of ES), the small one stays under
64 bytes: one bitmap word and a half."""
import numpy as np
import pytest

import flv_model as fm
import mp4_model as mm
import ts_model as tm
from easydarwin_amd import edgpu
from flv_model import KEY, PARAMS
from test_gpu_flv import check as flv_check
from test_gpu_mp4 import check as mp4_check
from test_gpu_ts import SMALL, check as ts_check, es_unit, layout

pytestmark = pytest.mark.gpu

SC = b"\x00\x00\x00\x01"
CHECK = {"ts": ts_check, "mp4": mp4_check, "flv": flv_check}
MODEL = {"ts": tm, "mp4": mm, "flv": fm}
SEQUENCE = [("ts", "large"), ("mp4", "large"), ("flv", "large"), ("mp4", "small"), ("ts", "small"), ("flv", "small"),
            ("flv", "large"), ("mp4", "large")]


def key_unit(n, k):
    """SPS, PPS and an IDR slice, n bytes together."""
    head = SC + bytes([0x67, 0x42, 0xC0, 0x1E, 0x9A, 0x74, 0x0B, 0x43, 0x6C, 0x10 + k]) + SC + bytes([0x68, 0xCE, 0x3C, 0x80 + k])
    return head + es_unit(n - len(head), k, 0x65)


def two_nal_unit(n, k):
    """n >= 33 bytes with a start code inside."""
    return es_unit(21, k) + es_unit(n - 21, k + 1)


def inputs(call):
    """The two inputs of call `call`: [[(es bytes, rtp_ts, flags)]] per stream, the time moving on with the calls."""
    t = 90000 * call
    large = [[(key_unit(500, 1), t, KEY | PARAMS), (b"", t + 3000, 0), (two_nal_unit(540, 2), t + 6000, 0)],
             [(key_unit(96, 3), t + 7, KEY | PARAMS), (b"", t + 3007, 0), (two_nal_unit(952, 4), t + 6007, 0)]]
    small = [[(es_unit(22, 5), t, KEY), (es_unit(33, 6), t + 3000, 0)]]
    assert len(layout(large)[0]) == 2048 + 40 and len(layout(small)[0]) < 64
    return dict(large=large, small=small)


@pytest.mark.parametrize("device", [False, True])
def test_interleaved_muxes_on_one_context(device):
    """Every call's bytes, rows and new states against the model of its format (the checks of the
    formats' own tests); each format carries its own state rows from its previous call.  device: the
    fragmented-MP4 and FLV calls read a device `es` and write a device `out` -- the caller's buffers, only
    the tables are the context's."""
    with edgpu.Context(**SMALL) as c:
        states = {f: [m.new_state(), m.new_state()] for f, m in MODEL.items()}
        for call, (f, size) in enumerate(SEQUENCE):
            per_stream = inputs(call)[size]
            kinds = dict(es_kind="device", out_kind="device") if device and f != "ts" else {}
            new = CHECK[f](c, None, per_stream, states=states[f][:len(per_stream)], what=f"call {call}: {f}, {size}", **kinds)
            states[f][:len(per_stream)] = new
        assert all(s["started"] == 1 for f in states for s in states[f])
        assert [len(c.kernel_times(k)) for k in (6, 7, 8)] == [2, 3, 3]


def model_drain(fmt, data, units, streams, kept):
    """What Context.tap_drain_<fmt> owes for a plain drain (data, units, streams): (bytes, a mask of the
    bytes inside the runs, the model's rows...).  `kept`: the model's states by (session, track); they move on."""
    keys = [(int(st["session"]), int(st["track"])) for st in streams]
    outs = []
    for fill in (0x00, 0xFF):                               # the bytes between two runs are nobody's
        st = [dict(kept.get(k, MODEL[fmt].new_state())) for k in keys]
        kw = {} if fmt == "ts" else dict(fill=fill)
        outs.append(MODEL[fmt].mux(None, data.tobytes(), units, streams, st, **kw))
    kept.update(zip(keys, st))
    a, b = (np.frombuffer(o[0], dtype=np.uint8) for o in outs)
    return (a, a == b) + tuple(outs[0][1:-1])


def same_rows(got, want):
    assert len(got) == len(want)
    for k, (r, w) in enumerate(zip(got, want)):
        assert {f: int(r[f]) for f in w} == w, f"row {k}"


def test_drains_of_three_formats_on_one_context():
    """Context.tap_drain_ts, _mp4 and _flv in turn on successive ticks of one trace, each against its
    model fed from a plain drain of a second context that ingests the same; then a tap_disable of one
    track: the next drain of every format starts that track anew."""
    import tap_traces as tt
    from test_gpu_tap import add, ingest
    from test_mp4_init import CASES, PPS
    sps = CASES["baseline 640x480"][0]
    sessions = [[[sps, PPS, tt.nal(5, 900 + 100 * k + a)] if a % 6 == 0 else [tt.nal(1, 40 + 37 * a + k), tt.nal(1, 5)]
                 for a in range(36)] for k in range(2)]
    with edgpu.Context(**SMALL) as c, edgpu.Context(**SMALL) as plain:
        ids = [add(c) for _ in range(2)]
        assert [add(plain) for _ in range(2)] == ids
        packets = [tt.packetise(aus, mtu=700, stap=True, seq0=1000 * (k + 1))[0] for k, aus in enumerate(sessions)]
        kept = {"ts": {}, "mp4": {}, "flv": {}}
        for part in range(9):
            fmt = ("ts", "mp4", "flv")[part % 3]
            if part == 6:                                   # every format has run twice: its states are carried
                for x in (c, plain):
                    x.tap_disable(ids[0], 0)
                    x.tap_enable(ids[0], 0)
                for f in kept:                              # ... and this track's are dropped: started == 0 again
                    assert kept[f].pop((ids[0], 0))["started"] == 1
            batch = []
            for k, pk in enumerate(packets):
                lo, hi = len(pk) * part // 9, len(pk) * (part + 1) // 9
                batch += [(ids[k], 0, 10 * part, p) for p in pk[lo:hi]]
            for x in (c, plain):
                ingest(x, batch)
            data, units, streams = plain.tap_drain(flush=part == 8)
            assert len(streams) == 2 and len(units)
            want = model_drain(fmt, data, units, streams, kept[fmt])
            got = getattr(c, "tap_drain_" + fmt)(flush=part == 8)
            assert len(got[0]) == len(want[0]) and np.array_equal(got[0][want[1]], want[0][want[1]]), f"part {part}: {fmt} bytes"
            same_rows(got[1], want[2])
            if fmt == "mp4":
                same_rows(got[2], want[3])
            assert np.array_equal(got[-1], streams) and (fmt == "ts" or np.array_equal(got[-2], units))
