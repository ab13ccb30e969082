"""What the time_*.py tools share: the engine on a torch stream, blocks of back-to-back launches between two hipEvents
(torch's), the JSON writer -- and, for the timers of the image calls, their whole frame (Timer): the three arguments, the images and
the tensor pair, the copy that is the byte floor, the record of a measurement, the tear-down and the JSON envelope.  Importing it
puts the repository root on sys.path."""
import argparse
import json
import os
import sys
from statistics import median  # (also for a tool that needs the median before record(): time_turbulence.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def open_engine_on_stream(device=0):
    """(eng, stream): an Engine whose context launches on a torch stream of its own, which torch's events can time."""
    import torch
    import jello_amd
    eng = jello_amd.Engine(device)
    stream = torch.cuda.Stream(torch.device("cuda", device))
    eng.set_stream(stream.cuda_stream)
    return eng, stream


def timed(stream, launch, blocks, per_block, warmup=3):
    """us per launch in each of `blocks` blocks of `per_block` back-to-back launches, after `warmup` launches."""
    import torch
    for _ in range(warmup):
        launch()
    times = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(per_block):
            launch()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / per_block)
    return times


def write_json(path, payload):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(payload, f, indent=1)
    print("wrote", path)


class Timer:
    """The frame of a time_<call>.py tool.  Timer(tool, blocks, per_block, out) parses [--blocks] [--per-block] [--out] with the
    tool's defaults (`out`: a file name under profiles/) and opens the engine on a stream; `eng` and `results` are the tool's to use."""

    def __init__(self, tool, blocks, per_block, out):
        ap = argparse.ArgumentParser()
        ap.add_argument("--blocks", type=int, default=blocks)
        ap.add_argument("--per-block", type=int, default=per_block)
        ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
        self.tool, self.args = tool, ap.parse_args()
        self.eng, self.stream = open_engine_on_stream()
        self.results, self.images = [], set()

    def upload(self, bits, *ids):
        """The (H, W, 4) f16 bits as the image of every one of `ids`; finish() frees them."""
        for i in ids:
            self.eng.upload_image(i, bits)
            self.images.add(i)

    def tensors(self, width, height, dtype="float16"):
        """Two torch tensors of an image's shape on the stream -- zeros and ones -- which copy() copies between."""
        import torch
        with torch.cuda.stream(self.stream):
            self.ta = torch.zeros((height, width, 4), dtype=getattr(torch, dtype), device="cuda")
            self.tb = torch.ones((height, width, 4), dtype=getattr(torch, dtype), device="cuda")

    def copy(self, rect=None):
        """The byte floor of a call on `rect` (x, y, w, h; None: the whole image): a launch that copies the rectangle's view from
        one tensor to the other on the stream -- 8 B read and 8 B written per texel."""
        import torch
        ta, tb, stream = self.ta, self.tb, self.stream
        if rect is None:
            def launch():
                with torch.cuda.stream(stream):
                    tb.copy_(ta)
        else:
            x, y, w, h = rect

            def launch():  # (the views are taken per launch, as the committed profiles' runs took them)
                with torch.cuda.stream(stream):
                    tb[y:y + h, x:x + w].copy_(ta[y:y + h, x:x + w])
        return launch

    def timed(self, launch):
        return timed(self.stream, launch, self.args.blocks, self.args.per_block)

    def record(self, r, times, floor=None, more=None):
        """One result: r gains us_median / us_blocks / us_spread, with a floor copy_us_median / ratio_to_copy, then what
        more(median) returns; appended, printed as a JSON line; returns the median."""
        med = median(times)
        r.update({"us_median": round(med, 3), "us_blocks": [round(t, 3) for t in times], "us_spread": round(max(times) - min(times), 3)})
        if floor is not None:
            r.update({"copy_us_median": round(floor, 3), "ratio_to_copy": round(med / floor, 2)})
        if more is not None:
            r.update(more(med))
        self.results.append(r)
        print(json.dumps(r), flush=True)
        return med

    def finish(self, note, size=None, **extra):
        """Frees the images, restores the stream, closes the engine and writes the file: tool, device, blocks, per_block, size (where
        the tool has one), note, the tool's `extra` keys, results."""
        import torch
        for i in sorted(self.images):
            self.eng.free_image(i)
        self.eng.sync()
        self.eng.set_stream(None)
        self.eng.close()
        out = {"tool": self.tool, "device": torch.cuda.get_device_name(0), "blocks": self.args.blocks, "per_block": self.args.per_block}
        if size is not None:
            out["size"] = size
        write_json(self.args.out, dict(out, note=note, **extra, results=self.results))
