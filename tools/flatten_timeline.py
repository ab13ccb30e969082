"""When the waves of k_flatten_items run which unit of work (variant library built with -DFL_TIMING; JELLO_HIP_LIB selects it):
every wave records the wall clock at kernel entry and around every unit it runs, and whether the unit was heavy (Euler jobs).
ONE frame after the warm-up; the report is markdown (profiles/flatten_shares.md keeps it).
    make -C jello_amd/csrc VARIANT=fltime EXTRA=-DFL_TIMING
    JELLO_HIP_LIB=jello_amd/libjello_hip_fltime.so python tools/flatten_timeline.py [c3|c2] [paths] [size] [raw.npy]"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jello_amd
from jello_amd import scenes
from jello_amd.engine import RUN_DISPATCHES
which = sys.argv[1] if len(sys.argv) > 1 else "c3"
paths = int(sys.argv[2]) if len(sys.argv) > 2 else {"c3": 100_000, "c2": 300}[which]
size = int(sys.argv[3]) if len(sys.argv) > 3 else {"c3": 4096, "c2": 1024}[which]
s, p = {"c3": scenes.scene_c3, "c2": scenes.scene_c2}[which](paths, size)
eng = jello_amd.Engine(0)
p.bump = s.bump_sizes(p.width, p.height)
rec, bump, attempts = eng.render(s, p, retain=True)
assert bump["failed"] == 0
fn = eng.hip.jh_debug_flatten_timeline
fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
dims = (ctypes.c_uint32 * 3)()
assert fn(None, 0, 1, dims) == 0
n_waves, words, khz = int(dims[0]), int(dims[1]), int(dims[2])
eng.run(rec, RUN_DISPATCHES)
eng.sync()
raw = np.zeros(n_waves * words, np.uint64)
assert fn(raw.ctypes.data, raw.size, 0, None) == 0
eng.close()
if len(sys.argv) > 4:  # the raw records, for a closer look
    np.save(sys.argv[4], raw.reshape(n_waves, words))

tl = raw.reshape(n_waves, words)
ran = tl[:, 0] != 0
t0 = int(tl[ran, 0].min())
us = lambda ticks: (np.asarray(ticks, np.float64) - t0) * 1e3 / khz
cap = (words - 2) // 3
units = tl[:, 1].astype(np.int64)
assert units.max() <= cap, "a wave ran %d units, the timeline keeps %d" % (units.max(), cap)
starts, ends, heavy, rank, info = [], [], [], [], []  # one entry per unit; rank = how many heavy units the wave had run before
for w in np.flatnonzero(ran):
    h = 0
    for k in range(int(units[w])):
        a, b = int(tl[w, 2 + 3 * k]), int(tl[w, 3 + 3 * k])
        info.append(int(tl[w, 4 + 3 * k]))
        hv = (a >> 63) != 0
        starts.append(a & ((1 << 63) - 1)); ends.append(b); heavy.append(hv); rank.append(h if hv else -1)
        h += hv
starts, ends, heavy, rank = us(starts), us(ends), np.array(heavy), np.array(rank)
info = np.array(info, np.int64)
pieces, steps, bail = info & 0xffff, (info >> 16) & 0x7fff, (info >> 31) & 1
end_all = float(ends.max())
print("scene %s, %d paths, %d x %d: %d lines; clock %d kHz" % (which, paths, size, size, bump["lines"], khz))
print()
print("- waves that ran: %d of %d launched slots; units: %d heavy, %d light; kernel entry to last unit's end: %.1f us"
      % (ran.sum(), n_waves, heavy.sum(), (~heavy).sum(), end_all))
print("- last wave enters the kernel at %.1f us" % float(us(tl[ran, 0]).max()))
for r in range(int(rank.max()) + 1):
    m = rank == r
    print("- heavy unit no. %d of its wave: %d waves; starts %.1f .. %.1f us, ends %.1f .. %.1f us, mean duration %.1f us"
          % (r + 1, m.sum(), starts[m].min(), starts[m].max(), ends[m].min(), ends[m].max(), (ends[m] - starts[m]).mean()))
dur = ends - starts
hd = dur[heavy]
print("- duration of a heavy unit: " + ", ".join("p%d %.1f" % (q, np.percentile(hd, q)) for q in (0, 10, 50, 90, 99, 100)) + " us; %d gave up (sequential walk)" % bail[heavy].sum())
print("- pieces of a heavy unit: " + ", ".join("p%d %.0f" % (q, np.percentile(pieces[heavy], q)) for q in (0, 10, 50, 90, 100))
      + "; steps of phase A: " + ", ".join("p%d %.0f" % (q, np.percentile(steps[heavy], q)) for q in (0, 10, 50, 90, 100)))
if heavy.sum() > 2:
    print("- correlation of a heavy unit's duration with its pieces %.2f, with its steps of phase A %.2f, with its start time %.2f"
          % (np.corrcoef(hd, pieces[heavy])[0, 1], np.corrcoef(hd, steps[heavy])[0, 1], np.corrcoef(hd, starts[heavy])[0, 1]))
    first = rank == 0
    cu = np.repeat(np.flatnonzero(ran), units[ran])[first] // 4  # workgroup of the wave
    per_wg = np.array([dur[first][cu == c].mean() for c in np.unique(cu)])
    print("- first heavy units: spread of the workgroups' mean durations p0 %.1f, p50 %.1f, p100 %.1f us (within a workgroup: mean range %.1f us)"
          % (per_wg.min(), np.median(per_wg), per_wg.max(), np.mean([np.ptp(dur[first][cu == c]) for c in np.unique(cu)])))
    # the workgroups in the order of their dispatch, in quarters (with four workgroups per CU: the first, ..., fourth on its CU)
    n_wg = int(np.flatnonzero(ran).max()) // 4 + 1
    quarter = np.minimum(cu * 4 // n_wg, 3)
    unit_wave = np.repeat(np.flatnonzero(ran), units[ran])
    last_end = np.array([ends[unit_wave == w].max() for w in np.flatnonzero(ran)])
    wave_quarter = np.minimum((np.flatnonzero(ran) // 4) * 4 // n_wg, 3)
    print("- by quarter of the dispatch order: mean duration of the first heavy unit "
          + " / ".join("%.1f" % dur[first][quarter == q].mean() for q in range(4) if (quarter == q).any())
          + " us; mean end of a wave's last unit " + " / ".join("%.1f" % last_end[wave_quarter == q].mean() for q in range(4) if (wave_quarter == q).any())
          + " us; units per wave " + " / ".join("%.2f" % units[ran][wave_quarter == q].mean() for q in range(4) if (wave_quarter == q).any()))
m = ~heavy
if m.any():
    print("- light units: %d; start %.1f .. %.1f us, end %.1f .. %.1f us, mean duration %.2f us"
          % (m.sum(), starts[m].min(), starts[m].max(), ends[m].min(), ends[m].max(), (ends[m] - starts[m]).mean()))
print()
print("| bucket (us) | waves inside a heavy unit | inside a light unit | share of the %d waves busy |" % ran.sum())
print("|---|---|---|---|")
edges = np.linspace(0.0, end_all, 11)
for i in range(10):
    lo, hi = edges[i], edges[i + 1]
    inside = np.clip(np.minimum(ends, hi) - np.maximum(starts, lo), 0.0, None) / (hi - lo)  # time-averaged over the bucket
    print("| %.1f - %.1f | %.0f | %.0f | %.0f %% |" % (lo, hi, inside[heavy].sum(), inside[~heavy].sum(), 100.0 * inside.sum() / ran.sum()))
