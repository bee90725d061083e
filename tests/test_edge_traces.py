"""CPU: the directed edge traces (tests/edge_traces.py).  On every one the clean-room restatement
(oracle/relay_model) must equal the REAL reference reflector (oracle/_ref/ref_harness) byte for
byte and the committed digest (tests/golden/edge_traces.json, which pins the GPU box, where the
reference tree is absent, to the reference), and the trace must reach every edge it claims: a
trace that misses its edge fails here, not silently on the GPU."""
import hashlib
import json
import os

import pytest

from easydarwin_amd.trace import read_capture, split_wire_image
from edge_traces import (B_COUNTS, B_JOIN_COUNT, CHUNK, E_RTCP_LENS, EDGE_TRACES, PATCHING, PLAIN, edge_trace)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_traces.json")


def fixture(name):
    with open(GOLD) as f:
        return json.load(f)["traces"][name]


def _run(binary, trace, tmp_path, tag):
    import subprocess
    t, c = tmp_path / f"{tag}.edtr", tmp_path / f"{tag}.edcp"
    t.write_bytes(trace)
    subprocess.run([binary, str(t), str(c)], check=True, stderr=subprocess.DEVNULL, timeout=300)
    return c.read_bytes()


def _pow2_at_least(n):
    return 1 << (n - 1).bit_length()


def check_lenphase(name, tr, c, cap):
    assert c["kernel"] == (PATCHING if name.endswith("mixed") else PLAIN)
    assert c["lengths"] == list(range(0, 2062)) + [3000, 65535]
    assert c["packets"] == 2063                                     # all but the empty one take a slot
    assert c["pairs"] == {(ph, m) for ph in range(8) for m in range(16)}
    assert c["tick_first_phases"] == set(range(8))
    assert all(v.n_packets == 2063 for k, v in cap.items() if k[2] == 0)


def check_chunks(name, tr, c, cap):
    kern = PATCHING if name.endswith("tcp") else PLAIN
    assert c["kernel"] == kern
    assert c["counts"] >= {(n, kern) for n in B_COUNTS}
    assert c["starts"] == {(p, kern) for p in range(34)}
    assert c["in_chunk_starts"] == set(range(CHUNK[kern]))
    for sub, p, idr in c["joins"]:                                   # the joiner's window starts at the IDR
        ss = cap[(sub, 0, 0)]
        assert hashlib.sha256(split_wire_image(ss.data, ss.tcp)[0]).hexdigest() == idr, (sub, p)
        assert ss.n_packets == (B_JOIN_COUNT - p) + B_JOIN_COUNT * (33 - p) + c["tail"], (sub, p)


def check_wrap(name, tr, c, cap):
    assert c["kernel"] == (PATCHING if "mixed" in name else PLAIN)
    assert c["chunk_wrap_phases"] == set(range(8))
    assert c["chunk_wraps"] >= 48 and c["words"] >= 48 * c["ring_words"]      # dozens of wraps
    assert c["slot_wraps"] >= 1
    assert c["packet_ring_chunk_splits"] >= 1
    assert c["max_tick_words"] < c["ring_words"] and c["max_tick_packets"] <= 64   # nobody lags: a tick fits
    assert c["max_len"] == (2043 if name.endswith("2043") else 65535)


def check_neighbours(name, tr, c, cap):
    assert c["kernel"] == (PATCHING if name.endswith("patch") else PLAIN)
    assert c["nwork"] >= 4096
    assert 2 * c["contrast_pairs"] >= c["pairs"]
    assert bool(c["rewrite"]) == name.endswith("patch")


def check_rewrite_edges(name, tr, c, cap):
    assert c["kernel"] == PATCHING
    assert c["rtp_lens"] >= set(range(1, 25)) and len(c["rtp_lens"]) >= 60
    assert c["rtcp"] == {(pt, n) for pt in (200, 201) for n in E_RTCP_LENS}
    assert c["rtcp_burst"] >= 33
    for chunk in CHUNK.values():                # an SR of >= 20 bytes first, last and interior in a chunk
        at = {p % chunk for p in c["sr_positions"]}
        assert 0 in at and chunk - 1 in at and at - {0, chunk - 1}
    assert c["rtcp_burst"] - 1 in c["sr_positions"]                 # and last of a short chunk
    rw = c["rewrite"]
    assert any(sd and c["seq0"] + sd > 0xFFFF for sd, _, _ in rw.values())
    assert any(td and c["ts0"] + td > 0xFFFFFFFF for _, td, _ in rw.values())
    assert any(sd and not td for sd, td, _ in rw.values()) and any(td and not sd for sd, td, _ in rw.values())
    tcp_of = {k[0]: v.tcp for k, v in cap.items()}
    assert {tcp_of[s] for s, p in rw.items() if p[2] is not None} == {0, 1}       # an SSRC on UDP and on TCP
    assert all(any(s not in rw for s in (3 * k + 1, 3 * k + 2, 3 * k + 3)) for k in range(2))   # an identity output each
    # the reference relays every threshold length on both kinds (what the GPU test then transforms)
    for kind, want in ((0, {7, 8, 11, 12, 19, 20}), (1, {4, 7, 8, 12, 19, 20})):
        got = {len(p) for k, v in cap.items() if k[2] == kind for p in split_wire_image(v.data, v.tcp)}
        assert got >= want, (kind, sorted(want - got))


def check_aktt(name, tr, c, cap):
    # the ring holds a joiner's second at the stripped lengths, with more to spare
    # than one ingest round's trailers (256 x 16 B); at the unstripped lengths it does not
    assert c["held_stripped"] + 4096 <= c["ring_bytes"] < c["held_unstripped"]
    # and grown to the reference's 10-s retention, the two layouts would end a doubling apart
    assert _pow2_at_least(2 * c["total_stripped"]) < _pow2_at_least(2 * c["total_unstripped"])
    assert c["tagged"] >= 3900
    assert all(v.n_packets > 1000 for k, v in cap.items() if k[2] == 0)


CHECKS = {"lenphase": check_lenphase, "chunks": check_chunks, "wrap": check_wrap, "neighbours": check_neighbours,
          "rewrite": check_rewrite_edges, "aktt": check_aktt}


@pytest.mark.parametrize("name", list(EDGE_TRACES))
def test_edge_trace_reaches_its_edges_and_oracle_matches_reference(name, oracle_bins, tmp_path):
    if oracle_bins["ref"] is None:
        pytest.skip("oracle/_ref/ref_harness not built (reference tree absent)")
    tr, claims = edge_trace(name)
    trace = tr.to_bytes()
    fix = fixture(name)
    assert hashlib.sha256(trace).hexdigest() == fix["trace_sha256"], "trace generator drifted from the fixture"
    ref = _run(oracle_bins["ref"], trace, tmp_path, "ref")
    same = _run(oracle_bins["port"], trace, tmp_path, "port") == ref       # (no pytest diff of MBs)
    assert same
    assert hashlib.sha256(ref).hexdigest() == fix["capture_sha256"]
    CHECKS[name.split("_")[0]](name, tr, claims, read_capture(ref))


@pytest.mark.parametrize("name", list(EDGE_TRACES))
def test_edge_trace_fixture_is_current(name):
    """Without the reference tree too: the generator still gives the trace the digest was taken on."""
    assert hashlib.sha256(edge_trace(name)[0].to_bytes()).hexdigest() == fixture(name)["trace_sha256"]
