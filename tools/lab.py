#!/usr/bin/env python3
"""The GPU probes of this project as one command (run on the GPU box): variant libraries, bench lines, kernel statistics,
counter passes, differential splits, forced-path parity runs, soaks, sweeps.  Every build and every GPU program goes
through tools/steps.py: a variant library is built beside the product one (which no probe ever rebuilds), every step
has a time limit, and the first step that fails, faults, aborts or runs out of time ends the run.

  tools/lab.py [--plan] [--prebuilt] [--out DIR] SUBCOMMAND ...
                                                        (--plan: print what would be built and run as JSON, run nothing;
                                                         --prebuilt: build nothing, the variant libraries are there already;
                                                         <out> is DIR, lab_out/ in the repository by default)
    bench NAME... [-- bench args]                       one `bench.py --full` line per library
    kstats [--tolerate] [--full] PATTERN NAME... [-- bench args]
                                                        kernel times (rocprofv3 --kernel-trace --stats); two rounds for several
                                                        libraries; --full: the long one-library form that keeps kernel_stats.csv
    counters PATTERN "CTR CTR ..." NAME... [-- bench args]     per-launch averages of the kernels that match PATTERN
    counters KERNEL,KERNEL|- issue|mem|flatten NAME... [-- bench args]     the named counter groups (-: the group's own kernels)
    fine-counters COMMIT [bench args]                   -> <out>/fine_counters[_<scene>].json
    split fine|flatten|lines [--commit ID] [-- bench args]     differential builds of one kernel
    parity NAME... [-- pytest args]                     forced-path builds through the GPU tests and a fuzz soak
    soak [--base SEED]                                  16 000 fuzz frames in two groups of four processes, then determinism
    soak-ffcheck FIRST PER [NPROC] [--seconds S]        tools/soak_flatten_fast.py on the check build, NPROC <= 5 processes
    sweep flatten|pc|coarse|bbox|fine_clip [bench args] one variant library per configuration, then its measurement
    overlap [bench args]                                kernel trace of two frames in flight -> <out>/overlap.txt
    collect COMMIT [--part 1|2]                         everything profiles/ holds for one state of the code
NAME is `product`, an entry of VARIANTS, a sweep configuration (fl_r32_w4_b5) or a library copied in as
jello_amd/libjello_hip_NAME.so."""
import argparse
import collections
import contextlib
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import steps  # noqa: E402

R = steps.ROOT
PY = sys.executable
BENCH = [PY, os.path.join(R, "bench.py")]

# name -> (EXTRA, results wrong by construction, what it is for)
FINE_SKIP = {1: "without stage 3 (crossing-pixel formula)", 2: "without stage 4 (row walk, y_edge terms)",
             3: "without stages 2 + 3 (pair evaluation)", 4: "without batches (stages 1-4)", 5: "without the solid-colour composite",
             6: "FLOOR: real PTCL / windows / pair and crossing-pixel counts, only the arithmetic of the output (y-part per pair, formula per crossing pixel, two packed adds per segment, finalisation, composite, store)"}
VARIANTS = {"skip%d" % n: ("-DJH_VARIANT_BUILD -DFINE_SKIP=%d" % n, True, "k_fine_area " + what) for n, what in FINE_SKIP.items()}
VARIANTS.update({
    "flnob": ("-DFL_SPLIT_NO_B", True, "k_flatten_items without phase B (pieces)"),
    "flnoab": ("-DFL_SPLIT_NO_A -DFL_SPLIT_NO_B", True, "k_flatten_items without phases A + B (subdivision)"),
    "lsplit1": ("-DFL_LSPLIT=1", True, "k_flatten_lines without the Euler evaluation"),
    "lsplit2": ("-DFL_LSPLIT=2", True, "k_flatten_lines without its stores"),
    "ffcheck": ("-DFL_FAST_CHECK", False, "k_flatten_items evaluates the pinned sequence beside the fast subdivision test and counts contradictions"),
    # forced paths: results do not change
    "tinycap": ("-DFLQ_STACK=96u -DFLQ_LEAVES=80u", False, "k_flatten_items: tiny LDS stack / piece list, most batches take the sequential fall-back"),
    "maxlevel2": ("-DFLQ_MAX_LEVEL=2u", False, "k_flatten_items: trees deeper than two levels take the fall-back"),
    "fbblocks2": ("-DFB_MAX_BLOCKS=2u", False, "k_flatten_bbox on two workgroups: every wave strides over many line ranges"),
    "home0": ("-DFL_SOAK_HOME0", False, "flatten's temporary in eight regions, every wave starts in region 0: regions fill up; its soak also runs with tight line buffers"),
    "split1": ("-DCOARSE_MAX_SPLIT=1u", False, "coarse: one workgroup per bin (64 tiles per wave), with and without clip layers"),
    "split2": ("-DCOARSE_MAX_SPLIT=2u", False, "coarse: two workgroups per bin"),
    "cache256": ("-DCOARSE_TILE_CACHE=256u", False, "coarse: the smallest Tile cache, every batch worked on in many windows"),
    "split8cache300": ("-DCOARSE_MAX_SPLIT=8u -DCOARSE_TILE_CACHE=300u", False, "coarse: eight workgroups per bin on a small Tile cache"),
    "msdirect5": ("-DMS_FORCE_DIRECT_ABOVE=5u", False, "multisampled fine: the walk at the fill for every segment with more than 5 touched pixels"),
    "mscap64": ("-DMS_CAP_OVERRIDE=64u", False, "multisampled fine: lists of 64 touched pixels (fills over many batches, the wholesale clear)"),
    "parwg16pool1": ("-DCOARSE_PAR_WG_PER_CU=16u -DCOARSE_POOL_CHUNKS=1u", False, "coarse with clip layers: sixteen workgroups per CU, an arena share of one chunk"),
})

# what `parity` runs per forced-path library: test files, then (first seed, count, extra environment) of each fuzz soak
_P, _K, _C = "tests/test_gpu_parity.py", "tests/test_gpu_kat.py", "tests/test_gpu_clip.py"
PARITY = {"tinycap": ([_P], [(100, 300, {})]), "maxlevel2": ([_P], [(100, 300, {})]), "fbblocks2": ([_P], [(100, 300, {})]),
          "home0": ([_P], [(100, 300, {}), (100, 200, {"TIGHT_LINES": "1"})]),
          "split1": ([_P, _K, _C], [(100, 200, {}), (940000, 300, {})]),
          "split2": ([_P, _K], [(100, 200, {})]), "cache256": ([_P, _K], [(100, 200, {})]), "split8cache300": ([_P, _K], [(100, 200, {})]),
          "msdirect5": ([_P, _K, _C], [(940000, 300, {})]), "mscap64": ([_P, _K, _C], [(940000, 300, {})]),
          "parwg16pool1": ([_P, _K, _C], [(940000, 300, {})])}

# family -> (variant name, EXTRA, configurations): performance-only macros, results do not change
SWEEPS = {"flatten": ("fl_r%d_w%d_b%d", "-DFL_REFILL_LANES=%du -DFL_WAVES_PER_EU=%d -DFL_BLOCKS_PER_CU=%d",
                      [(32, 4, 5), (32, 4, 4), (32, 4, 6), (32, 4, 8), (32, 4, 10), (32, 3, 4), (32, 3, 5), (32, 3, 6)]),
          "pc": ("pc_%d", "-DPC_BIG_PATH=%du", [(64,), (128,), (256,), (1024,)]),
          "coarse": ("co_c%d_w%d_s%d", "-DCOARSE_TILE_CACHE=%du -DCOARSE_WG_PER_CU=%du -DCOARSE_MAX_SPLIT=%du",
                     [(1536, 2, 16), (1536, 4, 16), (768, 6, 16), (512, 8, 16)]),
          "bbox": ("fb_t%d", "-DFB_TARGET_WAVES=%du", [(256,), (1024,), (2048,), (8192,)]),
          "fine_clip": ("fc_w%d", "-DFINE_CLIP_WAVES_PER_EU=%d", [(2,), (3,), (4,)])}
SWEEP_VARIANTS = {name % c: (extra % c, False, "sweep " + fam) for fam, (name, extra, cfgs) in SWEEPS.items() for c in cfgs}

ISSUE_1 = "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES"
ISSUE_2 = "SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_INST_CYCLES_VMEM SQ_WAVES SQ_INSTS_SMEM SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS"
# group -> (output folder, counter passes, the group's own kernels); counters of one pass fit the hardware together
# (mem: only this pass -- the TCC_EA0_* / TCC_HIT / TA_* groups made rocprofv3 abort after its 300 s limit)
COUNTER_GROUPS = {
    "issue": ("pmc", [ISSUE_1, ISSUE_2], None),
    "mem": ("pmcmem", ["TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_LATENCY_sum TCC_TAG_STALL_sum TCC_BUSY_sum TCC_CYCLE_sum"], None),
    "flatten": ("flpmc", ["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY"],
                "k_flatten_classify,k_flatten_items,k_flatten_lines,k_flatten_bbox,k_pc_count,k_pc_paths,k_pc_emit,k_pc_rank_small,k_coarse,k_path_tiling,k_scan_lookback")}
FINE_PASSES = ["FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES",
               "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SMEM"]
# the bench run of a counter pass: one context, no graph, every extra frame is rows in the CSV
PMC_BENCH = "--steps 2 --warmup 1 --blocks 1 --min-seconds 0 --no-cpu-baseline --no-graph".split()


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def planning():
    return steps.PLAN is not None


def out(*p):
    return os.path.join(steps.OUT, *p)


def fresh(*p):
    d = out(*p)
    if not planning():
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    return d


def lib(name):
    extra, wrong, _ = VARIANTS.get(name) or SWEEP_VARIANTS.get(name) or (None, False, "")
    return steps.variant_lib(name, extra, wrong)


def rocprof(name, opts, program, seconds, raw, **kw):
    """rocprofv3 around one program: kernel trace only, plus --stats or ONE --pmc pass; run from /tmp as its scratch."""
    return steps.step(name, ["rocprofv3", "--kernel-trace"] + opts + ["--output-format", "csv", "-d", raw, "--"] + program, seconds,
                      env={"TMPDIR": "/tmp"}, cwd="/tmp", **kw)


def last_json(log):
    return json.loads([l for l in open(log, errors="replace") if l.startswith("{")][-1])


def tail(log, n=1):
    print("\n".join(open(log, errors="replace").read().splitlines()[-n:]))


def table(script, args, pattern=None):
    """profiles/kstats.py or profiles/pmc.py on CSV files (CPU only); the lines that match `pattern`."""
    text = subprocess.run([PY, os.path.join(R, "profiles", script)] + args, stdout=subprocess.PIPE, check=True).stdout.decode()
    text = "".join(l + "\n" for l in text.splitlines() if pattern is None or re.search(pattern, l))
    print(text, end="")
    return text


def counter_avgs(pattern, match, key=lambda name: name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0][:60]):
    """{key(kernel): {counter: average per launch}} of the rows of the counter CSVs under `pattern` whose kernel name `match` accepts."""
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(pattern):
        for r in csv.DictReader(open(f)):
            if match(r["Kernel_Name"]):
                agg[key(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return {k: {n: sum(x) / len(x) for n, x in sorted(c.items())} for k, c in agg.items()}


@contextlib.contextmanager
def into(path):
    """What the block prints goes to `path` (collect keeps every table as a file)."""
    if planning():
        yield
    else:
        with open(path, "w") as f, contextlib.redirect_stdout(f):
            yield


# ---- step shapes -------------------------------------------------------------------------------------------------------
def bench(libs, args):
    for l in libs:
        log = steps.step("variants/" + l.name, BENCH + ["--full", "--no-cpu-baseline"] + args, 200, lib=l)
        if not planning():
            d = last_json(log)
            print(l.name, "frame", d["ms_per_step"], "one at a time", (d.get("one_frame_at_a_time") or {}).get("ms_per_step"), "fine", d["roofline"]["avg_ms"],
                  "stages", {k: round(v, 4) for k, v in d.get("stage_ms", {}).items()} if "stage_ms" in d else "")


def kstats(pattern, libs, args, tolerate=False):
    """Same-box A/B of kernel times, interleaved; one context, so that a kernel's duration is its own."""
    if tolerate and not any(l.changes_results for l in libs):
        sys.exit("--tolerate: none of these libraries has results that are wrong by construction")
    for rnd in (1, 2) if len(libs) > 1 else (1,):
        for l in libs:
            d = fresh("ab_" + l.name)
            rocprof("ab_%s/bench" % l.name, ["--stats"], BENCH + "--steps 20 --warmup 3 --blocks 2 --min-seconds 0 --no-cpu-baseline --in-flight 1".split() + args,
                    200, d + "/raw", lib=l, tolerate_failure=tolerate and l.changes_results)
            if not planning():
                print("== %s (round %d)" % (l.name, rnd))
                f = sorted(glob.glob(d + "/raw/*/*kernel_stats.csv"))
                table("kstats.py", [f[0], "60"], pattern) if f else print("(no kernel statistics)")
                shutil.rmtree(d + "/raw", ignore_errors=True)


def kprof(tag, l, args, pattern=None, summary=True):
    """Per-kernel device times of one bench configuration -> <out>/kprof_<tag>/kernel_stats.csv + a short table."""
    d = fresh("kprof_" + tag)
    log = rocprof("kprof_%s/bench" % tag, ["--stats"], BENCH + "--full --steps 20 --warmup 3 --no-cpu-baseline --in-flight 1".split() + args, 300, d + "/raw", lib=l)
    if planning():
        return
    shutil.copy(sorted(glob.glob(d + "/raw/*/*kernel_stats.csv"))[0], d + "/kernel_stats.csv")
    shutil.rmtree(d + "/raw")
    table("kstats.py", [d + "/kernel_stats.csv", "60"], pattern)
    if summary:
        j = last_json(log)
        print("ms_per_step", j["ms_per_step"], "value", j["value"])
        print({k: v for k, v in j["stage_ms"].items() if v > 0.02})


def counters(pattern, ctrs, libs, args):
    if ctrs in COUNTER_GROUPS:
        folder, passes, own = COUNTER_GROUPS[ctrs]
        ks = own if pattern == "-" else pattern
        assert ks, "this counter group has no kernels of its own: name them"
        for l in libs:
            d = fresh("%s_%s" % (folder, l.name))
            for i, grp in enumerate(passes, 1):
                rocprof("%s_%s/g%d" % (folder, l.name, i), ["--pmc"] + grp.split(), BENCH + PMC_BENCH + args, 300, "%s/g%d" % (d, i), lib=l)
                if not planning():
                    with open(d + "/summary.txt", "a") as f:
                        f.write(table("pmc.py", glob.glob("%s/g%d/*/*counter_collection.csv" % (d, i)) + ["--k=" + ks]))
                    shutil.rmtree("%s/g%d" % (d, i))
        return
    for l in libs:
        d = fresh("abc_" + l.name)
        rocprof("abc_%s/bench" % l.name, ["--pmc"] + ctrs.split(), BENCH + PMC_BENCH + ["--in-flight", "1"] + args, 300, d + "/raw", lib=l)
        if not planning():
            for k, c in counter_avgs(d + "/raw/*/*counter_collection.csv", lambda n: re.search(pattern, n)).items():
                print("==", l.name, k, {n: round(v) for n, v in c.items()})
            shutil.rmtree(d + "/raw")


def fine_counters(commit, args):
    """Counter summary of the fine kernel: separate passes (FETCH_SIZE and WRITE_SIZE do not fit one), then the static
    instruction mix priced with the measured issue costs (tools/fine_isa.sh, tools/isa_price.py)."""
    d = fresh("pmc_fine")
    for i, grp in enumerate(FINE_PASSES, 1):
        rocprof("pmc_fine/g%d" % i, ["--pmc"] + grp.split(), BENCH + PMC_BENCH + args, 300, "%s/g%d" % (d, i))
    steps.step("pmc_fine/isa", ["bash", os.path.join(R, "tools", "fine_isa.sh")], 300)
    if not planning():
        write_fine_counters(d, commit, R, args)


def write_fine_counters(out, commit, root, args):  # (bench.py reads profiles/fine_counters*.json: every key stays)
    import hashlib
    h = hashlib.sha256()
    for f in ("kernels_fine.hip", "kcommon.h", "dmath.h"):
        h.update(open(os.path.join(root, "jello_amd", "csrc", f), "rb").read())
    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default
    scene = opt("--scene", "c3")
    agg = collections.defaultdict(list)
    for f in glob.glob(out + "/g*/*/*counter_collection.csv"):
        for r in csv.DictReader(open(f)):
            if "k_fine_area" in r["Kernel_Name"]:
                agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    avg = {k: sum(v) / len(v) for k, v in agg.items()}
    fetch_kb, write_kb = avg.get("FETCH_SIZE"), avg.get("WRITE_SIZE")
    j = {"kernel": "k_fine_area", "scene": scene, "paths": int(opt("--paths", 100000 if scene == "c3" else 30000)),
         "size": int(opt("--size", 4096 if scene == "c3" else 2048)), "aa": opt("--aa", "area"), "commit": commit,
         "kernel_source_sha256": h.hexdigest(),
         "source": "rocprofv3 --kernel-trace --pmc <group> (one pass per group: FETCH_SIZE | WRITE_SIZE | SQ_* x2), averages over the launches of bench.py --steps 2 --warmup 1 --no-graph",
         "counters_avg_per_launch": {k: round(v, 1) for k, v in sorted(avg.items())},
         "FETCH_SIZE_KB": fetch_kb, "WRITE_SIZE_KB": write_kb,
         "hbm_bytes_per_launch": None if fetch_kb is None or write_kb is None else int(fetch_kb * 1024 * 2 + write_kb * 1024),
         "correction": "bytes = KB * 1024; gfx950: FETCH_SIZE doubled (MI355X_MICROARCH.md: wide coalesced reads are tallied at half) -- an upper bound here, the kernel mixes 4/8/16-byte-per-lane loads; WRITE_SIZE exact",
         "valu_insts_per_launch": avg.get("SQ_INSTS_VALU"), "salu_insts_per_launch": avg.get("SQ_INSTS_SALU"),
         "lds_insts_per_launch": avg.get("SQ_INSTS_LDS"), "simds": 1024, "clock_ghz": 2.4,
         "tiles": (int(opt("--size", 4096 if scene == "c3" else 2048)) // 16) ** 2}
    try:
        inst = "ILi%dELb%dELb%dE" % ({"area": 0, "msaa8": 8, "msaa16": 16}[opt("--aa", "area")], 0 if scene in ("c3", "c1", "c2") else 1,
                                     0 if scene in ("c3", "c1", "c2") else 1)
        pr = json.loads(subprocess.check_output([sys.executable, root + "/tools/isa_price.py", "/tmp/asm/fine.s", "k_fine_area" + inst]).decode())
        j["isa_static_mix"] = pr
        j["valu_cycles_per_inst_static_mix"] = pr["valu_cycles_per_inst_static_mix"]
        j["issue_rates_source"] = "profiles/r03_ubench_issue_rates.txt (tools/ubench/valu3.hip on an MI355X): 2.2 / 4.2 / 8.1 cycles of a SIMD per wave64 instruction by class; SALU 4.08"
    except Exception as e:  # noqa: BLE001
        j["isa_static_mix_error"] = str(e)
    name = "fine_counters.json" if scene == "c3" else "fine_counters_%s.json" % scene
    json.dump(j, open(os.path.join(steps.OUT, name), "w"), indent=1)
    print(json.dumps(j, indent=1))


def split_fine(commit, args):
    """Per-stage split of k_fine_area: each skipN library leaves one part of the kernel out (its results are wrong, only
    its counters and times are read) -> <out>/fine_split.json"""
    d = fresh("fine_split")
    libs = [lib("product")] + [lib("skip%d" % n) for n in range(1, 7)]
    for n, l in enumerate(libs):
        steps.step("fine_split/bench%d" % n, BENCH + ["--full", "--no-cpu-baseline"] + args, 300, lib=l, tolerate_failure=l.changes_results)
        rocprof("fine_split/p%d" % n, ["--pmc"] + "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_LDS_BANK_CONFLICT".split(),
                BENCH + PMC_BENCH + args, 300, "%s/p%d" % (d, n), lib=l, tolerate_failure=l.changes_results)
    if planning():
        return
    names = dict(FINE_SKIP)
    names[0] = "product library"
    rows = []
    for n in range(7):
        avg = counter_avgs("%s/p%d/*/*counter_collection.csv" % (d, n), lambda k: "k_fine_area" in k, key=lambda k: "").get("", {})
        try:
            ms = last_json("%s/bench%d.log" % (d, n))["roofline"]["avg_ms"]
        except Exception:  # noqa: BLE001  (a library whose frames are wrong may fail the bench's own check)
            ms = None
        rows.append({"variant": n, "what": names[n], "fine_ms": ms, "counters": {k: round(v) for k, v in sorted(avg.items())}})
    tiles = 65536.0
    base = rows[0]["counters"]
    for r in rows[1:]:
        c = r["counters"]
        r["delta_per_tile"] = {k: round((base.get(k, 0) - c.get(k, 0)) / tiles, 1) for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS")}
        if r["fine_ms"] is not None and rows[0]["fine_ms"] is not None:
            r["delta_ms"] = round(rows[0]["fine_ms"] - r["fine_ms"], 4)
    j = {"kernel": "k_fine_area", "commit": commit, "method": "differential builds (FINE_SKIP=n variant libraries, results wrong by construction), rocprofv3 --pmc per launch, bench.py stage time", "rows": rows}
    json.dump(j, open(out("fine_split.json"), "w"), indent=1)
    for r in rows:
        print(r["variant"], r["what"], r["fine_ms"], r.get("delta_per_tile"), r.get("delta_ms"))


def split_flatten():
    """Where k_flatten_items' instructions go: without phase B (pieces), without phases A + B (subdivision)."""
    for v, l in [("product", lib("product")), ("nob", lib("flnob")), ("noab", lib("flnoab"))]:
        d = fresh("flsplit_" + v)
        rocprof("flsplit_" + v, ["--pmc"] + "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES".split(), BENCH + PMC_BENCH, 300, d, lib=l,
                tolerate_failure=l.changes_results)
        if not planning():
            print("== " + v)
            table("pmc.py", glob.glob(d + "/*/*counter_collection.csv") + ["--k=k_flatten_items,k_flatten_lines"])


def split_lines():
    """Where k_flatten_lines' time goes: without the Euler evaluation (lsplit1), without the stores (lsplit2)."""
    for l in [lib("product"), lib("lsplit1"), lib("lsplit2")]:
        d = fresh("lsplit_" + l.name)
        rocprof("lsplit_%s/stats" % l.name, ["--stats"], BENCH + "--steps 10 --warmup 2 --blocks 1 --min-seconds 0 --no-cpu-baseline --no-graph --in-flight 1".split(),
                300, d + "/t", lib=l, tolerate_failure=l.changes_results)
        rocprof("lsplit_%s/pmc" % l.name, ["--pmc"] + "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY".split(),
                BENCH + PMC_BENCH + ["--in-flight", "1"], 300, d + "/p", lib=l, tolerate_failure=l.changes_results)
        if not planning():
            print("== " + l.name)
            table("kstats.py", [sorted(glob.glob(d + "/t/*/*kernel_stats.csv"))[0], "60"], "k_flatten")
            table("pmc.py", glob.glob(d + "/p/*/*counter_collection.csv") + ["--k=k_flatten_lines"])
            shutil.rmtree(d + "/t")
            shutil.rmtree(d + "/p")


def parity(names, pytest_args):
    for n in names:
        if n not in PARITY:
            sys.exit("parity: %s is no forced-path build (%s)" % (n, " ".join(PARITY)))
    for l in [lib(n) for n in names]:
        files, soaks = PARITY[l.name]
        planning() or print("[%s]" % VARIANTS[l.name][0], flush=True)
        logs = [steps.step("parity_%s/pytest" % l.name, [PY, "-m", "pytest"] + files + ["-m", "gpu", "-x", "-q"] + pytest_args, 500, lib=l)]
        for i, (first, count, env) in enumerate(soaks):
            logs.append(steps.step("parity_%s/soak%d" % (l.name, i), [PY, "tools/parity_soak.py", str(first), str(count)], 300, lib=l, env=env))
        if not planning():
            for log in logs:
                tail(log)


def soak(base):
    """Fuzz scenes (all coverage modes, clips, gradients, images) through the HIP pipeline and the oracle in four processes,
    the same with the smallest line buffers the frames fit, then run-to-run determinism at full size."""
    for tag, first, per, seconds, env in (("fuzz", base, 1500, 1000, {}), ("tight", base + 10000, 500, 900, {"TIGHT_LINES": "1"})):
        for log in steps.group([dict(name="soak/%s_%d" % (tag, i), argv=[PY, "tools/parity_soak.py", str(first + i * per), str(per)], seconds=seconds, env=env)
                                for i in range(4)]):
            planning() or tail(log)
    log = steps.step("soak/determinism", [PY, "tools/determinism.py"], 600)
    planning() or tail(log, 6)


def soak_ffcheck(first, per, nproc, seconds):
    if nproc > 5:  # (the soak is bound by building the fuzz scenes on the host, not by the GPU)
        sys.exit("at most 5 processes")
    l = lib("ffcheck")
    for log in steps.group([dict(name="ffsoak_%d_%d" % (first, i), argv=[PY, "tools/soak_flatten_fast.py", str(first + i * per), str(per)], seconds=seconds, lib=l)
                            for i in range(nproc)]):
        planning() or tail(log)


def sweep(family, args):
    name, _, cfgs = SWEEPS[family]
    libs = [lib(name % c) for c in cfgs]  # every build before the first measurement
    for l in libs:
        if family in ("flatten", "pc"):
            stage, opts = {"flatten": ("flatten", "--full --steps 20 --warmup 2 --blocks 3 --no-cpu-baseline --no-graph"),
                           "pc": ("path_count", "--full --steps 10 --warmup 2 --no-cpu-baseline")}[family]
            log = steps.step("sweep_%s/%s" % (family, l.name), BENCH + opts.split() + args, 200, lib=l)
            if not planning():
                d = last_json(log)
                print(l.name, d["ms_per_step"], d["stage_ms"].get(stage))
        elif family == "coarse":
            for s in ("c3", "c4"):
                planning() or print(l.name, s)
                kprof("sw", l, ["--scene", s] + args, "k_coarse", summary=False)
        elif family == "bbox":
            for p in ("100000", "20000"):
                planning() or print(l.name, "paths=" + p)
                kprof("bbs", l, ["--paths", p] + args, "k_flatten_bbox", summary=False)
        else:  # fine_clip: occupancy of the clip / blend instantiations of k_fine_area on C4
            log = steps.step("sweep_fine_clip/" + l.name, [PY, "tools/time_configs.py"], 300, lib=l)
            if not planning():
                print(l.name)
                print("".join(x for x in open(log, errors="replace") if "C4" in x), end="")


def overlap(args):
    """How the kernels of two frames in flight share the device -> <out>/overlap.txt"""
    d = fresh("overlap")
    rocprof("overlap/bench", [], BENCH + "--full --steps 60 --warmup 3 --blocks 1 --min-seconds 0 --no-cpu-baseline".split() + args, 300, d + "/raw")
    if planning():
        return
    f = sorted(glob.glob(d + "/raw/*/*kernel_trace.csv"))[0]
    with open(f) as src, open(out("overlap_head.txt"), "w") as dst:
        dst.writelines(src.readlines()[:2])
    with open(out("overlap.txt"), "w") as o, open(out("overlap_err.txt"), "w") as e:
        subprocess.run([PY, os.path.join(R, "tools", "overlap_trace.py"), f], stdout=o, stderr=e)
    shutil.rmtree(d + "/raw")
    print(open(out("overlap.txt")).read(), end="")


def collect(commit, part):
    """-> <out>/collect/.  Part 1: counters, kernel statistics, bench lines; part 2: the splits, PTCL statistics, other scenes,
    frames in flight (two parts, because one visit to the GPU box is limited in time)."""
    o = fresh("collect") if part != 2 else out("collect")
    planning() or os.makedirs(o, exist_ok=True)
    product = lib("product")

    def copy(pattern, dst):
        for f in [] if planning() else glob.glob(pattern):
            shutil.copy(f, dst)
    if part != 2:
        # counters first: the bench lines below report roofline.traffic from profiles/fine_counters*.json only if those were
        # measured on the kernel sources being run (here: on the box's copy of profiles/; copy collect/fine_counters*.json home)
        for s, a in (("c3", []), ("c4", ["--scene", "c4"]), ("c4n", ["--scene", "c4n"])):
            with into("%s/pmc_%s.log" % (o, s)):
                fine_counters(commit, a)
        copy(out("fine_counters*.json"), os.path.join(R, "profiles"))
        for s in ("c3", "c4", "c4n"):
            with into("%s/%s_summary.txt" % (o, s)):
                kprof("col_" + s, product, ["--scene", s])
            copy(out("kprof_col_" + s, "kernel_stats.csv"), "%s/%s_kernel_stats.csv" % (o, s))
            steps.step("collect/%s_bench" % s, BENCH + ["--full", "--scene", s], 300)
        for aa in ("msaa8", "msaa16"):
            steps.step("collect/c3_%s_bench" % aa, BENCH + ["--full", "--aa", aa, "--no-cpu-baseline"], 300)
    if part == 1:
        return
    with into(o + "/fine_split.log"):
        split_fine(commit, [])
    copy(out("fine_split.json"), o)
    copy(out("fine_counters*.json"), o)
    for s in ("c3", "c4", "c4n"):
        steps.step("collect/ptcl_stats_" + s, [PY, "tools/ptcl_stats.py", s], 300)
    steps.step("collect/other_scenes_configs", [PY, "tools/time_configs.py"], 300)
    steps.step("collect/other_scenes_shapes", [PY, "tools/time_shapes.py"], 300)
    # the small configurations as bench lines, the counters of the flatten and tile-stage kernels, the splits of the flatten kernels
    for s in ("c1", "c2"):
        steps.step("collect/%s_bench" % s, BENCH + ["--full", "--scene", s, "--no-cpu-baseline"], 300)
    with into(o + "/pmc_flatten_tile_kernels.txt"):
        counters("-", "flatten", [product], [])
    with into(o + "/flatten_split.txt"):
        split_flatten()
    with into(o + "/lines_split.txt"):
        split_lines()
    for s in ("c3", "c4", "c4n"):
        steps.step("collect/frames_in_flight_" + s, [PY, "tools/frames_in_flight.py", "--scene", s, "--max-in-flight", "3"], 250)
    # if the library of the round before was built from its own sources and copied in as libjello_hip_r05.so: every kernel against it
    if os.path.exists(os.path.join(R, "jello_amd", "libjello_hip_r05.so")):
        libs = [lib("r05"), product]
        with into(o + "/ab_r05_vs_r06.txt"):
            for pattern, a in (("k_", []), ("k_", ["--scene", "c4"]), ("k_fine|k_coarse|k_clip", ["--scene", "c4n"]), ("k_fine", ["--aa", "msaa8"]), ("k_fine", ["--aa", "msaa16"])):
                kstats(pattern, libs, a)


def main(argv):
    argv, extra = (argv[:argv.index("--")], argv[argv.index("--") + 1:]) if "--" in argv else (argv, [])
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--out", default=steps.OUT)
    ap.add_argument("--prebuilt", action="store_true")
    sub = ap.add_subparsers(dest="cmd", required=True)

    def cmd(name, *positional):
        p = sub.add_parser(name)
        p.add_argument("--plan", action="store_true", default=argparse.SUPPRESS)
        for a in positional:
            p.add_argument(a)
        return p
    cmd("bench").add_argument("names", nargs="+")
    p = cmd("kstats", "pattern")
    p.add_argument("--tolerate", action="store_true")
    p.add_argument("--full", action="store_true")
    p.add_argument("names", nargs="+")
    cmd("counters", "pattern", "ctrs").add_argument("names", nargs="+")
    cmd("fine-counters", "commit")
    p = cmd("split")
    p.add_argument("kind", choices=("fine", "flatten", "lines"))
    p.add_argument("--commit", default="unknown")
    cmd("parity").add_argument("names", nargs="+")
    cmd("soak").add_argument("--base", type=int, default=920000)
    p = cmd("soak-ffcheck")
    p.add_argument("first", type=int)
    p.add_argument("per", type=int)
    p.add_argument("nproc", type=int, nargs="?", default=4)
    p.add_argument("--seconds", type=int, default=1000)
    p = cmd("sweep")
    p.add_argument("family", choices=sorted(SWEEPS))
    cmd("overlap")
    cmd("collect", "commit").add_argument("--part", type=int, choices=(1, 2))
    a, bare = ap.parse_known_args(argv)
    if bare and a.cmd not in ("fine-counters", "sweep", "overlap"):  # (these take bench arguments bare, as the scripts before them did)
        ap.error("unrecognized arguments: %s (bench / pytest arguments go behind --)" % " ".join(bare))
    steps.OUT, steps.PREBUILT = os.path.abspath(a.out), a.prebuilt
    if a.plan:
        steps.PLAN = []
    rest = bare + extra

    def go():
        if a.cmd == "bench":
            bench([lib(n) for n in a.names], rest)
        elif a.cmd == "kstats" and a.full:
            len(a.names) == 1 or sys.exit("kstats --full takes one library")
            kprof(a.names[0], lib(a.names[0]), rest, a.pattern)
        elif a.cmd == "kstats":
            kstats(a.pattern, [lib(n) for n in a.names], rest, a.tolerate)
        elif a.cmd == "counters":
            counters(a.pattern, a.ctrs, [lib(n) for n in a.names], rest)
        elif a.cmd == "fine-counters":
            fine_counters(a.commit, rest)
        elif a.cmd == "split":
            {"fine": lambda: split_fine(a.commit, rest), "flatten": split_flatten, "lines": split_lines}[a.kind]()
        elif a.cmd == "parity":
            parity(a.names, rest)
        elif a.cmd == "soak":
            soak(a.base)
        elif a.cmd == "soak-ffcheck":
            soak_ffcheck(a.first, a.per, a.nproc, a.seconds)
        elif a.cmd == "sweep":
            sweep(a.family, rest)
        elif a.cmd == "overlap":
            overlap(rest)
        elif a.cmd == "collect":
            collect(a.commit, a.part)
    steps.run(go)
    if planning():
        json.dump(steps.PLAN, sys.stdout, indent=1)
        print()


if __name__ == "__main__":
    main(sys.argv[1:])
