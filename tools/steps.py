"""The one place under tools/ that builds a variant library or starts a GPU program (tools/lab.py holds what to run).

  variant_lib(name, extra)   make VARIANT=name EXTRA=extra -> jello_amd/libjello_hip_<name>.so; the product library is never built here
  step(name, argv, seconds)  one fresh child under `timeout -k 10 seconds`, output in <OUT>/<name>.log, JELLO_HIP_LIB from `lib`
  group(steps)               up to 16 such children side by side, all awaited
  run(main)                  runs main(); the first step in trouble (time limit, abort, segmentation fault, GPU memory fault)
                             or failed ends the tool: exit 3 / 1, nothing is started after it, nothing is tried again
With PLAN set to a list nothing runs: builds, steps and groups are recorded there (lab.py --plan prints them as JSON)."""
import collections
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "lab_out")  # (lab.py --out DIR puts it elsewhere)
PLAN = None
PREBUILT = False  # variant libraries are taken as they lie there (built where the compiler is, run where the GPU is)
GROUP_CAP = 16
FAULT_TEXT = b"an illegal memory access was encountered"
# (`timeout` passes its child's exit status on and dies of the signal its child died of: 137 / -9 is the kill behind -k or anyone's)
TROUBLE = {124: "time limit", 137: "killed", -9: "killed", 134: "abort", -6: "abort", 139: "segmentation fault", -11: "segmentation fault"}

# name, path (None: the product library, no JELLO_HIP_LIB), whether its results are wrong by construction
Lib = collections.namedtuple("Lib", "name path changes_results")


class StepFailed(Exception):
    code = 1


class GpuTrouble(StepFailed):
    code = 3


def variant_lib(name, extra="", changes_results=False):
    if name == "product":
        if PLAN is None and not os.path.exists(os.path.join(ROOT, "jello_amd", "libjello_hip.so")):
            raise StepFailed("jello_amd/libjello_hip.so is missing: build it with `make -C jello_amd/csrc -j8` (no tool does)")
        return Lib(name, None, False)
    assert name.isidentifier(), name
    lib = Lib(name, os.path.join(ROOT, "jello_amd", "libjello_hip_%s.so" % name), changes_results)
    if PLAN is not None:
        PLAN.append({"build": name, "extra": extra})
    elif extra is None or PREBUILT:  # (extra None: a library from other sources, copied in beside the product one)
        if not os.path.exists(lib.path):
            raise StepFailed("%s: no such library%s" % (lib.path, "" if PREBUILT else " and no table entry to build it from"))
    else:
        cmd = ["make", "-s", "-C", os.path.join(ROOT, "jello_amd", "csrc"), "-j8", "VARIANT=" + name, "EXTRA=" + extra]
        log = _log("build_" + name)
        with open(log, "wb") as f:
            if subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT).returncode:
                raise StepFailed("build %s: failed (%s)\n%s" % (name, " ".join(cmd), _tail(log, 5)))
    return lib


def _log(name):
    path = os.path.join(OUT, name + ".log")
    if PLAN is None:
        os.makedirs(os.path.dirname(path), exist_ok=True)
    return path


def _tail(log, n=8):
    with open(log, "rb") as f:
        return b"\n".join(f.read().splitlines()[-n:]).decode(errors="replace")


def _start(name, argv, seconds, lib=None, env=None, tolerate_failure=False, cwd=ROOT):
    lib = lib or Lib("product", None, False)
    if tolerate_failure and not lib.changes_results:
        raise ValueError("step %s: a failure is tolerated only for a library whose results are wrong by construction, not %s" % (name, lib.name))
    add = dict(env or {})
    if lib.path:
        add["JELLO_HIP_LIB"] = lib.path
    s = {"step": name, "argv": list(argv), "env": add, "seconds": int(seconds), "log": _log(name), "cwd": cwd, "tolerate_failure": tolerate_failure}
    if PLAN is None:
        child_env = {k: v for k, v in os.environ.items() if k != "JELLO_HIP_LIB"}
        child_env.update(add)
        with open(s["log"], "wb") as f:
            s["proc"] = subprocess.Popen(["timeout", "-k", "10", str(s["seconds"])] + s["argv"], stdout=f, stderr=subprocess.STDOUT,
                                         stdin=subprocess.DEVNULL, env=child_env, cwd=cwd)
    return s


def _finish(s):
    """Waits for a started step; returns None, or the exception its status calls for."""
    rc = s.pop("proc").wait()
    with open(s["log"], "rb") as f:
        faulted = FAULT_TEXT in f.read()
    what = TROUBLE.get(rc) or ("GPU memory fault (exit %d)" % rc if faulted else None)
    if what:
        return GpuTrouble("step %s: TROUBLE: %s\n%s" % (s["step"], what, _tail(s["log"])))
    if rc and not s["tolerate_failure"]:
        return StepFailed("step %s: FAILED: exit %d\n%s" % (s["step"], rc, _tail(s["log"])))
    return None


def step(name, argv, seconds, **kw):
    """Returns the path of the step's log."""
    s = _start(name, argv, seconds, **kw)
    if PLAN is not None:
        PLAN.append(s)
    else:
        err = _finish(s)
        if err:
            raise err
    return s["log"]


def group(steps):
    """steps: keyword dictionaries of step().  Returns the logs; raises after ALL have ended, trouble before failure."""
    if len(steps) > GROUP_CAP:
        raise ValueError("a group of %d: at most %d processes may use the GPU side by side" % (len(steps), GROUP_CAP))
    started = [_start(**kw) for kw in steps]
    if PLAN is not None:
        PLAN.append({"group": started})
    else:
        errs = [e for e in [_finish(s) for s in started] if e]
        if errs:
            raise type(max(errs, key=lambda e: e.code))("\n".join(str(e) for e in errs))
    return [s["log"] for s in started]


def run(main):
    try:
        main()
    except StepFailed as e:
        print(e, file=sys.stderr)
        print("-- ended there: nothing more is started" + (", and nothing on this GPU until the cause is known" if e.code == 3 else ""), file=sys.stderr)
        sys.exit(e.code)
