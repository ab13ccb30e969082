"""What the time_*.py tools share: the engine on a torch stream, blocks of back-to-back launches between two hipEvents
(torch's), the JSON writer.  Importing it puts the repository root on sys.path."""
import json
import os
import sys

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
