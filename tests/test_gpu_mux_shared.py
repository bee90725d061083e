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


def model_drain(fmt, data, units, streams, kept, cfg=None):
    """What Context.tap_drain_<fmt> owes for a plain drain (data, units, streams): (bytes, a mask of the
    bytes inside the runs, the model's rows...).  `kept`: the model's states by (session, track); they move on.
    cfg: the model's Config (None: the defaults)."""
    keys = [(int(st["session"]), int(st["track"])) for st in streams]
    outs = []
    for fill in (0x00, 0xFF):                               # the bytes between two runs are nobody's
        st = [dict(kept.get(k, MODEL[fmt].new_state())) for k in keys]
        kw = {} if fmt == "ts" else dict(fill=fill)
        outs.append(MODEL[fmt].mux(cfg, data.tobytes(), units, streams, st, **kw))
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


# ---- the growth paths of Context._drain_and_mux: 64 stream rows, 4096 unit rows, a 1-MiB device ES, a 1-MiB output ----

MIB = 1 << 20


def one_packet_units(n, seq0, ts0, size, key_every=0):
    import tap_traces as tt
    return [tt.header(seq0 + k, ts0 + 3000 * k, True) + tt.nal(5 if key_every and k % key_every == 0 else 1, size, fill=k)
            for k in range(n)]


def same_drain(fmt, got, want, units, streams, what):
    assert len(got[0]) == len(want[0]) and np.array_equal(got[0][want[1]], want[0][want[1]]), f"{what}: {fmt} bytes"
    same_rows(got[1], want[2])
    if fmt == "mp4":
        same_rows(got[2], want[3])
    assert np.array_equal(got[-1], streams) and (fmt == "ts" or np.array_equal(got[-2], units)), what


def grown_drain(fmt, per_session, crossed):
    """per_session: [[packet]] -- one tapped session each on two fresh contexts (the caps are the context's:
    grown ones would hide the retry).  Context.tap_drain_<fmt> of one against the model fed from the plain
    drain of the other; `crossed(es bytes needed, units, streams, model output bytes)` says that the plain
    drain's sizes cross the threshold aimed at; then a small drain, which must still match: nothing was
    consumed twice and the states moved once."""
    from tap_model import TapModel
    from test_gpu_tap import add, expect, ingest, same, split
    with edgpu.Context(**SMALL) as c, edgpu.Context(**SMALL) as plain:
        ids = [add(c) for _ in per_session]
        assert [add(plain) for _ in per_session] == ids
        kept, taps = {}, [TapModel() for _ in ids]
        more = [one_packet_units(3, 40000, 1 << 30, 30 + k, key_every=2) for k in range(len(ids))]
        for step, traces in enumerate((per_session, more)):
            batch = [(s, 0, 1000 * step + j, p) for s, pk in zip(ids, traces) for j, p in enumerate(pk)]
            for x in (c, plain):
                ingest(x, batch)
            data, units, streams = plain.tap_drain()
            by_key = split(data, units, streams)                # the plain drain grows its buffers too: held to the tap model
            for s, m, pk in zip(ids, taps, traces):
                for j, p in enumerate(pk):
                    m.push(p, 1000 * step + j)
                same(by_key[(s, 0)], expect(m), f"plain drain {step}, session {s}")
            want = model_drain(fmt, data, units, streams, kept)
            need = sum((int(st["bytes"]) + 15) // 16 * 16 for st in streams)
            print(f"{fmt} drain {step}: es {need} units {len(units)} streams {len(streams)} out {len(want[0])}")
            assert len(streams) == len(ids) and len(units)
            assert step or crossed(need, len(units), len(streams), len(want[0]))
            same_drain(fmt, getattr(c, "tap_drain_" + fmt)(), want, units, streams, f"drain {step}")


@pytest.mark.parametrize("fmt", ["ts", "mp4", "flv"])
def test_binding_drain_of_65_taps(fmt):
    grown_drain(fmt, [one_packet_units(1 + k % 2, 100 * k, 5000 * k, 9 + k % 23, key_every=1 if k % 3 == 0 else 0) for k in range(65)],
                lambda es, units, streams, out: streams == 65 > 64 and units <= 4096 and es < MIB and out < MIB)


@pytest.mark.parametrize("fmt", ["ts", "mp4", "flv"])
def test_binding_drain_of_4097_units(fmt):
    grown_drain(fmt, [one_packet_units(4097, 65000, 7, 20, key_every=1000)],
                lambda es, units, streams, out: units == 4097 > 4096 and streams == 1 and es < MIB and out < MIB)


@pytest.mark.parametrize("fmt", ["ts", "mp4", "flv"])
def test_binding_drain_over_one_mib_of_es(fmt):
    """The device ES buffer is freed and a larger one allocated between the two drain attempts."""
    import tap_traces as tt
    pk, reached = tt.packetise([[tt.nal(5 if a % 10 == 0 else 1, 28000)] for a in range(40)], mtu=1400, seq0=500)
    assert "fu-middle" in reached and len(pk) == 840
    grown_drain(fmt, [pk], lambda es, units, streams, out: es > MIB and units <= 4096 and streams == 1)


@pytest.mark.parametrize("fmt", ["ts", "mp4", "flv"])
def test_binding_output_over_one_mib_from_less_es(fmt):
    """800 units of 1304 ES bytes: 188 bytes per 184 and the PES headers, 12 bytes per sample and 96 per
    fragment, or 20 bytes per tag take the output, and nothing else, over 1 MiB."""
    grown_drain(fmt, [one_packet_units(800, 300, 77, 1300, key_every=200)],
                lambda es, units, streams, out: es < MIB < out and units <= 4096 and streams == 1)
