"""Recording what the AAC audio tap drains (Context.aac_tap_drain under ADTS framing): a stream's
run of a drain is ADTS frame after ADTS frame, so it is appended to an .aac file as it stands.

Recorder writes <session>_<track>_<n>.aac per (session, track).  A file is cut only after a flush
(the drain that emptied the tap: nothing of the stream waits in a fragment chain), once `segment`
seconds of arrival time have passed since the file began; the next drain's frames start file n + 1.
"""
import json
import os


class Recorder:
    def __init__(self, out_dir, segment=300.0):
        self.out_dir, self.segment_ms = out_dir, int(segment * 1000)
        self.open = {}              # (session, track) -> [file object, entry, first arrival, last arrival]
        self.files = []
        self.frames = 0

    def push(self, data, frames, streams, flushed=False):
        """One drain: the bytes, AAC_FRAME_DTYPE rows and AAC_STREAM_DTYPE rows of Context.aac_tap_drain;
        `flushed` says the drain was made with flush=True."""
        self.frames += len(frames)
        for st in streams:
            key = (int(st["session"]), int(st["track"]))
            rows = frames[int(st["frame_first"]):int(st["frame_first"]) + int(st["frame_count"])]
            if len(rows):
                cur = self.open.get(key)
                if cur is None:
                    name = "%d_%d_%d.aac" % (key[0], key[1], sum(1 for f in self.files if f["stream"] == list(key)))
                    entry = {"file": name, "stream": list(key), "frames": 0, "bytes": 0, "discontinuities": 0}
                    self.files.append(entry)
                    cur = self.open[key] = [open(os.path.join(self.out_dir, name), "wb"), entry, int(rows[0]["arrival_ms"]), 0]
                off, n = int(st["offset"]), int(st["bytes"])
                cur[0].write(data[off:off + n].tobytes())
                cur[1]["frames"] += len(rows)
                cur[1]["bytes"] += n
                cur[1]["discontinuities"] += int(sum(1 for r in rows if int(r["flags"]) & 1))
                cur[3] = int(rows[-1]["arrival_ms"])
            cur = self.open.get(key)
            if flushed and cur and cur[3] - cur[2] >= self.segment_ms:
                cur[0].close()
                del self.open[key]

    def close(self):
        for cur in self.open.values():
            cur[0].close()
        self.open = {}
        with open(os.path.join(self.out_dir, "audio_index.json"), "w") as f:
            json.dump({"files": self.files, "frames": self.frames}, f)
