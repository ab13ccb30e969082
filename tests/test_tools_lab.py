"""tools/lab.py + tools/steps.py without a GPU: the plans of every subcommand against what the shell scripts they replaced ran
(transcribed by hand from those scripts: build flags, argv behind `timeout`, environment, seconds), the rules every plan keeps,
and the fault discipline of the runner with harmless stand-in children.

In the expectations $R is the repository, $O the tools' output folder, python3 the interpreter.  What differs from the scripts on
purpose: a counter group's folder carries the library's name (pmc_product, flpmc_product), tools/fine_isa.sh is started through
bash, the first bench step of the fine split has the 300 s of its neighbours, and sweeps / forced-path runs select a variant
library where the scripts rebuilt the product one."""
import inspect
import functools
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import steps  # noqa: E402


def _norm(x):
    if isinstance(x, str):
        x = "python3" if x == sys.executable else x
        return x.replace(steps.OUT, "$O").replace(ROOT, "$R")
    if isinstance(x, list):
        return [_norm(v) for v in x]
    if isinstance(x, dict):
        return {k: _norm(v) for k, v in x.items()}
    return x


@functools.lru_cache(maxsize=None)
def _plan(*args):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "lab.py"), "--plan"] + list(args), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return _norm(json.loads(r.stdout))


def _steps(plan):
    for rec in plan:
        for s in rec.get("group", [rec] if "step" in rec else []):
            yield s


def builds(*args):
    return [(r["build"], r["extra"]) for r in _plan(*args) if "build" in r]


def ran(*args):
    """(library, command line, environment besides the library, seconds) of every step, in order."""
    res = []
    for s in _steps(_plan(*args)):
        env = dict(s["env"])
        lib = env.pop("JELLO_HIP_LIB", "product")
        if lib != "product":
            assert lib.startswith("$R/jello_amd/libjello_hip_") and lib.endswith(".so"), lib
            lib = lib[len("$R/jello_amd/libjello_hip_"):-3]
        res.append((lib, " ".join(s["argv"]), env, s["seconds"]))
    return res


BENCH = "python3 $R/bench.py"
PMC_BENCH = BENCH + " --steps 2 --warmup 1 --blocks 1 --min-seconds 0 --no-cpu-baseline --no-graph"
TMP = {"TMPDIR": "/tmp"}


def prof(opts, folder, program):
    return "rocprofv3 --kernel-trace %s--output-format csv -d $O/%s -- %s" % (opts, folder, program)


# ---- 1. plans equal the scripts -------------------------------------------------------------------------------------------
def test_plan_bench():  # run_variants.sh
    assert builds("bench", "product", "split1") == [("split1", "-DCOARSE_MAX_SPLIT=1u")]
    assert ran("bench", "product", "split1") == [(v, BENCH + " --full --no-cpu-baseline", {}, 200) for v in ("product", "split1")]
    assert ran("bench", "product", "--", "--paths", "3000")[0][1] == BENCH + " --full --no-cpu-baseline --paths 3000"


def test_plan_kstats():  # ab_kernels.sh (AB_ARGS behind --), kprof.sh
    ab = BENCH + " --steps 20 --warmup 3 --blocks 2 --min-seconds 0 --no-cpu-baseline --in-flight 1 --scene c4"
    assert ran("kstats", "k_coarse", "product", "split1", "--", "--scene", "c4") == \
        [(v, prof("--stats ", "ab_%s/raw" % v, ab), TMP, 200) for _ in (1, 2) for v in ("product", "split1")]
    assert len(ran("kstats", "k_coarse", "split1")) == 1
    assert ran("kstats", "--full", ".", "product", "--", "--scene", "c4") == \
        [("product", prof("--stats ", "kprof_product/raw", BENCH + " --full --steps 20 --warmup 3 --no-cpu-baseline --in-flight 1 --scene c4"), TMP, 300)]
    assert all(s["cwd"] == "/tmp" for s in _steps(_plan("kstats", "k_coarse", "product", "split1")))


def test_plan_counters():  # ab_counters.sh, pmc.sh, pmc_mem.sh, pmc_flatten.sh
    assert builds("counters", "k_fine", "SQ_INSTS_VALU SQ_WAVE_CYCLES", "product", "skip2") == [("skip2", "-DJH_VARIANT_BUILD -DFINE_SKIP=2")]
    assert ran("counters", "k_fine", "SQ_INSTS_VALU SQ_WAVE_CYCLES", "product", "skip2", "--", "--scene", "c4") == \
        [(v, prof("--pmc SQ_INSTS_VALU SQ_WAVE_CYCLES ", "abc_%s/raw" % v, PMC_BENCH + " --in-flight 1 --scene c4"), TMP, 300) for v in ("product", "skip2")]
    issue = ["SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES",
             "SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_INST_CYCLES_VMEM SQ_WAVES SQ_INSTS_SMEM SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS"]
    assert ran("counters", "k_fine_area,k_coarse", "issue", "product", "--", "--scene", "c4") == \
        [("product", prof("--pmc %s " % g, "pmc_product/g%d" % i, PMC_BENCH + " --scene c4"), TMP, 300) for i, g in enumerate(issue, 1)]
    mem = "TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_LATENCY_sum TCC_TAG_STALL_sum TCC_BUSY_sum TCC_CYCLE_sum"
    assert ran("counters", "k_flatten_lines", "mem", "product") == [("product", prof("--pmc %s " % mem, "pmcmem_product/g1", PMC_BENCH), TMP, 300)]
    fl = "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY"
    assert ran("counters", "-", "flatten", "product") == [("product", prof("--pmc %s " % fl, "flpmc_product/g1", PMC_BENCH), TMP, 300)]


FINE_PASSES = ["FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES",
               "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SMEM"]


def fine_counters(args=""):
    return [("product", prof("--pmc %s " % g, "pmc_fine/g%d" % i, PMC_BENCH + args), TMP, 300) for i, g in enumerate(FINE_PASSES, 1)] + \
        [("product", "bash $R/tools/fine_isa.sh", {}, 300)]


def test_plan_fine_counters():  # pmc_fine.sh, which forwards its arguments
    assert ran("fine-counters", "abc1234", "--scene", "c4") == fine_counters(" --scene c4")
    assert builds("fine-counters", "abc1234") == []
    sh = open(os.path.join(TOOLS, "pmc_fine.sh")).read()
    assert 'lab.py" fine-counters "$@"' in sh and len(sh.strip().splitlines()) == 3


SKIPS = [("skip%d" % n, "-DJH_VARIANT_BUILD -DFINE_SKIP=%d" % n) for n in range(1, 7)]
SPLIT_CTRS = "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_LDS_BANK_CONFLICT"


def split_fine(args=""):
    return [s for n, v in enumerate(["product"] + [b[0] for b in SKIPS]) for s in
            ((v, BENCH + " --full --no-cpu-baseline" + args, {}, 300), (v, prof("--pmc %s " % SPLIT_CTRS, "fine_split/p%d" % n, PMC_BENCH + args), TMP, 300))]


FLSPLIT = [(v, prof("--pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES ", "flsplit_" + d, PMC_BENCH), TMP, 300)
           for v, d in (("product", "product"), ("flnob", "nob"), ("flnoab", "noab"))]
LSPLIT = [s for v in ("product", "lsplit1", "lsplit2") for s in
          ((v, prof("--stats ", "lsplit_%s/t" % v, BENCH + " --steps 10 --warmup 2 --blocks 1 --min-seconds 0 --no-cpu-baseline --no-graph --in-flight 1"), TMP, 300),
           (v, prof("--pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY ", "lsplit_%s/p" % v,
                    PMC_BENCH + " --in-flight 1"), TMP, 300))]


def test_plan_split():  # fine_split.sh, flatten_split.sh, lines_split.sh
    assert builds("split", "fine", "--commit", "abc", "--", "--scene", "c4") == SKIPS
    assert ran("split", "fine", "--commit", "abc", "--", "--scene", "c4") == split_fine(" --scene c4")
    assert builds("split", "flatten") == [("flnob", "-DFL_SPLIT_NO_B"), ("flnoab", "-DFL_SPLIT_NO_A -DFL_SPLIT_NO_B")]
    assert ran("split", "flatten") == FLSPLIT
    assert builds("split", "lines") == [("lsplit1", "-DFL_LSPLIT=1"), ("lsplit2", "-DFL_LSPLIT=2")]
    assert ran("split", "lines") == LSPLIT


P, K, C = "tests/test_gpu_parity.py", "tests/test_gpu_kat.py", "tests/test_gpu_clip.py"
TIGHT = {"TIGHT_LINES": "1"}
# soak_flatten_fallback.sh, soak_coarse_shapes.sh, soak_round6_shapes.sh: (name here, EXTRA, test files, soaks);
# -DCOARSE_MAX_SPLIT=1u is in two of the scripts and runs what both ran
FORCED = [("tinycap", "-DFLQ_STACK=96u -DFLQ_LEAVES=80u", [P], [("100 300", {})]),
          ("maxlevel2", "-DFLQ_MAX_LEVEL=2u", [P], [("100 300", {})]),
          ("fbblocks2", "-DFB_MAX_BLOCKS=2u", [P], [("100 300", {})]),
          ("home0", "-DFL_SOAK_HOME0", [P], [("100 300", {}), ("100 200", TIGHT)]),
          ("split1", "-DCOARSE_MAX_SPLIT=1u", [P, K, C], [("100 200", {}), ("940000 300", {})]),
          ("split2", "-DCOARSE_MAX_SPLIT=2u", [P, K], [("100 200", {})]),
          ("cache256", "-DCOARSE_TILE_CACHE=256u", [P, K], [("100 200", {})]),
          ("split8cache300", "-DCOARSE_MAX_SPLIT=8u -DCOARSE_TILE_CACHE=300u", [P, K], [("100 200", {})]),
          ("msdirect5", "-DMS_FORCE_DIRECT_ABOVE=5u", [P, K, C], [("940000 300", {})]),
          ("mscap64", "-DMS_CAP_OVERRIDE=64u", [P, K, C], [("940000 300", {})]),
          ("parwg16pool1", "-DCOARSE_PAR_WG_PER_CU=16u -DCOARSE_POOL_CHUNKS=1u", [P, K, C], [("940000 300", {})])]


@pytest.mark.parametrize("name,extra,files,soaks", FORCED, ids=[f[0] for f in FORCED])
def test_plan_parity(name, extra, files, soaks):
    assert builds("parity", name) == [(name, extra)]
    assert ran("parity", name) == [(name, "python3 -m pytest %s -m gpu -x -q" % " ".join(files), {}, 500)] + \
        [(name, "python3 tools/parity_soak.py " + s, env, 300) for s, env in soaks]
    assert ran("parity", name, "--", "-k", "c1 or clip_torture")[0][1] == "python3 -m pytest %s -m gpu -x -q -k c1 or clip_torture" % " ".join(files)
    assert all(s["cwd"] == "$R" for s in _steps(_plan("parity", name)))


def test_parity_table_is_the_forced_path_builds():
    import lab
    assert sorted(lab.PARITY) == sorted(f[0] for f in FORCED)
    assert all(not lab.VARIANTS[n][1] for n in lab.PARITY) and not lab.VARIANTS["ffcheck"][1]
    wrong = sorted(n for n, v in lab.VARIANTS.items() if v[1])
    assert wrong == sorted([b[0] for b in SKIPS] + ["flnob", "flnoab", "lsplit1", "lsplit2"])


def soak_plan(base):
    return [("product", "python3 tools/parity_soak.py %d 1500" % (base + i * 1500), {}, 1000) for i in range(4)] + \
        [("product", "python3 tools/parity_soak.py %d 500" % (base + 10000 + i * 500), TIGHT, 900) for i in range(4)] + \
        [("product", "python3 tools/determinism.py", {}, 600)]


def test_plan_soak():  # soak_round6.sh (SOAK_BASE -> --base); soak_round5.sh = the same shape from 820000
    assert ran("soak") == soak_plan(920000)
    assert ran("soak", "--base", "820000") == soak_plan(820000)
    assert [len(r.get("group", [])) for r in _plan("soak")] == [4, 4, 0]


def test_plan_soak_ffcheck():  # soak_flatten_fast.sh
    assert builds("soak-ffcheck", "200000", "500") == [("ffcheck", "-DFL_FAST_CHECK")]
    assert ran("soak-ffcheck", "200000", "500") == [("ffcheck", "python3 tools/soak_flatten_fast.py %d 500" % (200000 + i * 500), {}, 1000) for i in range(4)]
    assert ran("soak-ffcheck", "7", "10", "5", "--seconds", "600") == [("ffcheck", "python3 tools/soak_flatten_fast.py %d 10" % (7 + i * 10), {}, 600) for i in range(5)]
    assert [len(r.get("group", [])) for r in _plan("soak-ffcheck", "7", "10", "5")] == [0, 5]
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "lab.py"), "--plan", "soak-ffcheck", "7", "10", "6"], capture_output=True, text=True)
    assert r.returncode != 0 and "at most 5" in r.stderr


def kprof(lib, tag, args):
    return (lib, prof("--stats ", "kprof_%s/raw" % tag, BENCH + " --full --steps 20 --warmup 3 --no-cpu-baseline --in-flight 1 " + args), TMP, 300)


def test_plan_sweep_flatten():
    cfgs = ["32 4 5", "32 4 4", "32 4 6", "32 4 8", "32 4 10", "32 3 4", "32 3 5", "32 3 6"]
    names = ["fl_r%s_w%s_b%s" % tuple(c.split()) for c in cfgs]
    assert names[0] == "fl_r32_w4_b5"
    assert builds("sweep", "flatten") == [(n, "-DFL_REFILL_LANES=%su -DFL_WAVES_PER_EU=%s -DFL_BLOCKS_PER_CU=%s" % tuple(c.split())) for n, c in zip(names, cfgs)]
    assert ran("sweep", "flatten") == [(n, BENCH + " --full --steps 20 --warmup 2 --blocks 3 --no-cpu-baseline --no-graph", {}, 200) for n in names]


def test_plan_sweep_pc():
    assert builds("sweep", "pc") == [("pc_%d" % e, "-DPC_BIG_PATH=%du" % e) for e in (64, 128, 256, 1024)]
    assert ran("sweep", "pc", "--paths", "5000") == [("pc_%d" % e, BENCH + " --full --steps 10 --warmup 2 --no-cpu-baseline --paths 5000", {}, 200) for e in (64, 128, 256, 1024)]


def test_plan_sweep_coarse():
    cfgs = ["1536 2 16", "1536 4 16", "768 6 16", "512 8 16"]
    names = ["co_c%s_w%s_s%s" % tuple(c.split()) for c in cfgs]
    assert builds("sweep", "coarse") == [(n, "-DCOARSE_TILE_CACHE=%su -DCOARSE_WG_PER_CU=%su -DCOARSE_MAX_SPLIT=%su" % tuple(c.split())) for n, c in zip(names, cfgs)]
    assert ran("sweep", "coarse") == [kprof(n, "sw", "--scene " + s) for n in names for s in ("c3", "c4")]


def test_plan_sweep_bbox():
    assert builds("sweep", "bbox") == [("fb_t%d" % t, "-DFB_TARGET_WAVES=%du" % t) for t in (256, 1024, 2048, 8192)]
    assert ran("sweep", "bbox") == [kprof("fb_t%d" % t, "bbs", "--paths %d" % p) for t in (256, 1024, 2048, 8192) for p in (100000, 20000)]


def test_plan_sweep_fine_clip():
    assert builds("sweep", "fine_clip") == [("fc_w%d" % e, "-DFINE_CLIP_WAVES_PER_EU=%d" % e) for e in (2, 3, 4)]
    assert ran("sweep", "fine_clip") == [("fc_w%d" % e, "python3 tools/time_configs.py", {}, 300) for e in (2, 3, 4)]


def test_plan_overlap():  # overlap_trace.sh
    assert ran("overlap", "--in-flight", "2") == \
        [("product", prof("", "overlap/raw", BENCH + " --full --steps 60 --warmup 3 --blocks 1 --min-seconds 0 --no-cpu-baseline --in-flight 2"), TMP, 300)]


def test_plan_collect():  # collect_profiles.sh: PART=1, PART=2, both (no libjello_hip_r05.so here: no A/B against it)
    part1 = fine_counters() + fine_counters(" --scene c4") + fine_counters(" --scene c4n")
    for s in ("c3", "c4", "c4n"):
        part1 += [kprof("product", "col_" + s, "--scene " + s), ("product", BENCH + " --full --scene " + s, {}, 300)]
    part1 += [("product", BENCH + " --full --aa %s --no-cpu-baseline" % aa, {}, 300) for aa in ("msaa8", "msaa16")]
    part2 = split_fine()
    part2 += [("product", "python3 tools/ptcl_stats.py " + s, {}, 300) for s in ("c3", "c4", "c4n")]
    part2 += [("product", "python3 tools/time_configs.py", {}, 300), ("product", "python3 tools/time_shapes.py", {}, 300)]
    part2 += [("product", BENCH + " --full --scene %s --no-cpu-baseline" % s, {}, 300) for s in ("c1", "c2")]
    fl = "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY"
    part2 += [("product", prof("--pmc %s " % fl, "flpmc_product/g1", PMC_BENCH), TMP, 300)] + FLSPLIT + LSPLIT
    part2 += [("product", "python3 tools/frames_in_flight.py --scene %s --max-in-flight 3" % s, {}, 250) for s in ("c3", "c4", "c4n")]
    assert ran("collect", "abc", "--part", "1") == part1
    assert ran("collect", "abc", "--part", "2") == part2
    assert ran("collect", "abc") == part1 + part2
    assert builds("collect", "abc", "--part", "1") == []
    assert sorted(builds("collect", "abc")) == sorted(SKIPS + [("flnob", "-DFL_SPLIT_NO_B"), ("flnoab", "-DFL_SPLIT_NO_A -DFL_SPLIT_NO_B"),
                                                               ("lsplit1", "-DFL_LSPLIT=1"), ("lsplit2", "-DFL_LSPLIT=2")])


# ---- 2. rules that hold for every plan ------------------------------------------------------------------------------------
EVERY = [("bench", "product", "split1"), ("kstats", "k_", "product", "split1"), ("kstats", "--full", ".", "product"), ("kstats", "--tolerate", "k_fine", "product", "skip6"),
         ("counters", "k_fine", "SQ_INSTS_VALU", "product", "skip1"), ("counters", "k_fine_area", "issue", "product"), ("counters", "k_fine_area", "mem", "product"),
         ("counters", "-", "flatten", "product"), ("fine-counters", "abc"), ("split", "fine"), ("split", "flatten"), ("split", "lines"),
         ("parity",) + tuple(f[0] for f in FORCED), ("soak",), ("soak-ffcheck", "1", "2", "5"), ("sweep", "flatten"), ("sweep", "pc"), ("sweep", "coarse"),
         ("sweep", "bbox"), ("sweep", "fine_clip"), ("overlap",), ("collect", "abc")]


@pytest.mark.parametrize("args", EVERY, ids=[" ".join(a[:2]) for a in EVERY])
def test_rules_of_every_plan(args):
    plan = _plan(*args)
    import lab
    known = dict(lab.VARIANTS, **lab.SWEEP_VARIANTS)
    for rec in plan:
        if "build" in rec:  # a build is `make VARIANT=<name>`: never the product library
            assert rec["build"] and rec["build"] != "product" and rec["extra"] == known[rec["build"]][0]
            assert "FINE_SKIP" not in rec["extra"] or "-DJH_VARIANT_BUILD" in rec["extra"]
        assert len(rec.get("group", [])) <= 16
    for s in _steps(plan):
        assert isinstance(s["seconds"], int) and 0 < s["seconds"] <= 1000, s
        assert "make" not in s["argv"] and s["log"].startswith("$O/") and s["log"].endswith(s["step"] + ".log")
        lib = s["env"].get("JELLO_HIP_LIB", "")[len("$R/jello_amd/libjello_hip_"):-3]
        assert not s["tolerate_failure"] or known[lib][1], s  # only where the results are wrong by construction
        if s["argv"][0] == "rocprofv3":
            a = s["argv"]
            opts, program = a[:a.index("--")], a[a.index("--") + 1:]
            assert program[:2] == ["python3", "$R/bench.py"]
            assert opts[1] == "--kernel-trace" and not any(o.startswith("--") and o not in ("--kernel-trace", "--stats", "--pmc", "--output-format") for o in opts[1:]), opts
            assert not ("--pmc" in opts and "--stats" in opts)
        else:
            assert "rocprofv3" not in s["argv"]


def test_the_one_make_line_names_a_variant():
    src = open(os.path.join(TOOLS, "steps.py")).read() + open(os.path.join(TOOLS, "lab.py")).read()
    assert src.count('"make"') == 1 and '"make", "-s", "-C", os.path.join(ROOT, "jello_amd", "csrc"), "-j8", "VARIANT=" + name, "EXTRA=" + extra]' in src
    assert "exec" not in src.replace("sys.executable", "")
    assert inspect.signature(steps.step).parameters["seconds"].default is inspect.Parameter.empty


def test_group_cap():
    steps.PLAN = []
    try:
        one = dict(name="x", argv=["true"], seconds=1)
        steps.group([one] * 16)
        with pytest.raises(ValueError):
            steps.group([one] * 17)
    finally:
        steps.PLAN = None


# ---- 3. fault discipline, with harmless stand-in children -----------------------------------------------------------------
DRIVER = """
import json, sys
sys.path.insert(0, %r)
import steps
steps.OUT = sys.argv[1]
libs = {"wrong": steps.Lib("skip1", "/nonexistent/libjello_hip_skip1.so", True), "same": steps.Lib("split1", "/nonexistent/libjello_hip_split1.so", False)}
def kw(s):
    return dict(name=s["name"], argv=[sys.executable, "-c", s["code"]], seconds=s.get("seconds", 20), lib=libs.get(s.get("lib")), tolerate_failure=s.get("tolerate", False))
def main():
    for s in json.loads(sys.argv[2]):
        steps.group([kw(g) for g in s["group"]]) if "group" in s else steps.step(**kw(s))
steps.run(main)
""" % TOOLS


def drive(tmp_path, spec):
    (tmp_path / "driver.py").write_text(DRIVER)
    return subprocess.run([sys.executable, str(tmp_path / "driver.py"), str(tmp_path / "out"), json.dumps(spec)], capture_output=True, text=True, timeout=60)


def touch(tmp_path, name):
    return {"name": "after_" + name, "code": "open(%r, 'w')" % str(tmp_path / name)}


TROUBLE = {"segv_139": "import sys; sys.exit(139)", "abort_134": "import sys; sys.exit(134)",
           "killed_137": "import os; os.kill(os.getpid(), 9)", "fault_text_exit_0": "print('HIP error: an illegal memory access was encountered')"}


@pytest.mark.parametrize("kind", sorted(TROUBLE))
def test_trouble_ends_the_run(tmp_path, kind):
    r = drive(tmp_path, [{"name": "the_step_" + kind, "code": TROUBLE[kind], "lib": "wrong", "tolerate": True}, touch(tmp_path, "marker")])
    assert r.returncode == 3 and "the_step_" + kind in r.stderr and "TROUBLE" in r.stderr, r.stderr
    assert not (tmp_path / "marker").exists() and (tmp_path / "out" / ("the_step_%s.log" % kind)).exists()


def test_time_limit_is_trouble(tmp_path):
    r = drive(tmp_path, [{"name": "sleeper", "code": "import time; time.sleep(30)", "seconds": 1}, touch(tmp_path, "marker")])
    assert r.returncode == 3 and "sleeper" in r.stderr and "time limit" in r.stderr, r.stderr
    assert not (tmp_path / "marker").exists()


def test_failure_ends_the_run_unless_tolerated(tmp_path):
    fail = {"name": "failing", "code": "print('last words'); raise SystemExit(1)"}
    r = drive(tmp_path, [fail, touch(tmp_path, "marker")])
    assert r.returncode == 1 and "failing" in r.stderr and "FAILED" in r.stderr and "last words" in r.stderr
    assert not (tmp_path / "marker").exists()
    r = drive(tmp_path, [dict(fail, lib="wrong", tolerate=True), touch(tmp_path, "marker")])
    assert r.returncode == 0 and (tmp_path / "marker").exists(), r.stderr


def test_tolerance_is_refused_where_results_do_not_change(tmp_path):
    for lib in ("same", None):
        r = drive(tmp_path, [dict(touch(tmp_path, "started"), lib=lib, tolerate=True), touch(tmp_path, "marker")])
        assert r.returncode not in (0, 3) and "wrong by construction" in r.stderr
        assert not (tmp_path / "started").exists() and not (tmp_path / "marker").exists()
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "lab.py"), "--plan", "kstats", "--tolerate", "k_", "product", "split1"], capture_output=True, text=True)
    assert r.returncode != 0 and "wrong by construction" in r.stderr


def test_group_awaits_all_and_starts_nothing_after(tmp_path):
    slow = "import time; time.sleep(0.5); open(%r, 'w')"
    r = drive(tmp_path, [{"group": [{"name": "g/bad", "code": TROUBLE["segv_139"]}] + [{"name": "g/ok%d" % i, "code": slow % str(tmp_path / ("done%d" % i))} for i in range(3)]},
                         touch(tmp_path, "marker")])
    assert r.returncode == 3 and "g/bad" in r.stderr, r.stderr
    assert all((tmp_path / ("done%d" % i)).exists() for i in range(3)) and not (tmp_path / "marker").exists()
    r = drive(tmp_path, [{"group": [{"name": "g/fails", "code": "raise SystemExit(2)"}, {"name": "g/bad", "code": TROUBLE["abort_134"]}]}, touch(tmp_path, "marker")])
    assert r.returncode == 3 and "g/fails" in r.stderr and "g/bad" in r.stderr and not (tmp_path / "marker").exists()


def test_child_sees_the_library_and_no_stale_one(tmp_path, monkeypatch):
    monkeypatch.setenv("JELLO_HIP_LIB", "/stale.so")
    code = "import os; print('LIB=' + os.environ.get('JELLO_HIP_LIB', 'none'))"
    r = drive(tmp_path, [{"name": "a", "code": code}, {"name": "b", "code": code, "lib": "wrong"}])
    assert r.returncode == 0, r.stderr
    assert "LIB=none" in (tmp_path / "out" / "a.log").read_text() and "LIB=/nonexistent/libjello_hip_skip1.so" in (tmp_path / "out" / "b.log").read_text()


# ---- 5. the Makefile refuses other flags for the product library ------------------------------------------------------------
def test_makefile_guard(tmp_path):
    csrc = os.path.join(ROOT, "jello_amd", "csrc")
    for bad in (["EXTRA=-DX"], ["ATOMICOPT=-mllvm -amdgpu-atomic-optimizer-strategy=DPP"]):
        r = subprocess.run(["make", "-n", "-C", csrc] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and "VARIANT=" in r.stderr
    try:
        r = subprocess.run(["make", "-n", "-C", csrc, "VARIANT=guardcheck", "EXTRA=-DX"], capture_output=True, text=True)
        assert r.returncode == 0 and "-DX" in r.stdout and "libjello_hip_guardcheck.so" in r.stdout, r.stderr
    finally:
        shutil.rmtree(os.path.join(csrc, "obj_guardcheck"), ignore_errors=True)  # (`make -n` still writes the variant's .flags)
