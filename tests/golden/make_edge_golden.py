"""Regenerates tests/golden/edge_traces.json from the REAL reference: for every edge trace of
tests/edge_traces.py, the trace's sha256 and the sha256 of the capture oracle/_ref/ref_harness
(EasyDarwin's reflector compiled from the read-only reference sources) gives on it, after
requiring the restatement (oracle/relay_model) to give the same bytes.  A GPU box without the
reference tree is then still pinned to the reference on these traces.

Run where the reference tree is:  python tests/golden/make_edge_golden.py
The fixture is data only (digests and sizes); nothing here is reference source.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from easydarwin_amd.trace import read_capture  # noqa: E402
from edge_traces import EDGE_TRACES, edge_trace  # noqa: E402


def main():
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
    port = os.path.join(ROOT, "oracle", "relay_model")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for name in EDGE_TRACES:
            trace = edge_trace(name)[0].to_bytes()
            tpath = os.path.join(td, name + ".edtr")
            with open(tpath, "wb") as f:
                f.write(trace)
            rc, pc = tpath + ".ref", tpath + ".port"
            subprocess.run([ref, tpath, rc], check=True, stderr=subprocess.DEVNULL)
            subprocess.run([port, tpath, pc], check=True)
            rb, pb = open(rc, "rb").read(), open(pc, "rb").read()
            if rb != pb:
                raise SystemExit(f"{name}: port oracle disagrees with the reference")
            cap = read_capture(rb)
            out[name] = {"trace_sha256": hashlib.sha256(trace).hexdigest(), "trace_bytes": len(trace),
                         "capture_sha256": hashlib.sha256(rb).hexdigest(), "capture_bytes": len(rb),
                         "relayed_packets": sum(v.n_packets for v in cap.values()), "substreams": len(cap)}
            print(f"{name:20s} ok  {out[name]['relayed_packets']} packets, {len(cap)} sub-streams")
            for p in (tpath, rc, pc):
                os.remove(p)
    with open(os.path.join(HERE, "edge_traces.json"), "w") as f:
        json.dump({"generator": "tests/edge_traces.py (numpy PCG64, seed base 0xEA5D + 300)",
                   "source": "oracle/_ref/ref_harness (EasyDarwin reference reflector)",
                   "traces": out}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
