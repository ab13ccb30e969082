"""What the CPU tests of the C ABI share: include/jello_hip.h and the Go shim read as text, and the header's own numbers."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
JH = os.path.join(INCLUDE, "jello_hip.h")
GO = os.path.join(ROOT, "integration", "engine", "hip_engine", "hip_engine.go")


def header_arity():
    """name -> parameter count of every function declared in include/jello_hip.h."""
    with open(JH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(jh_\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def go_calls():
    """(name, argument count) of every C.jh_* call in the Go shim, by paren matching."""
    with open(GO) as f:
        text = f.read()
    calls = []
    for m in re.finditer(r"\bC\.(jh_\w+)\s*\(", text):
        i, depth, commas = m.end(), 1, 0
        start = i
        while depth:
            ch = text[i]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                commas += 1
            i += 1
        body = text[start:i - 1].strip()
        calls.append((m.group(1), 0 if not body else commas + 1))
    return calls


def c_values(expressions):
    """The integer values of C expressions over include/jello_hip.h and include/jello_formats.h (enumerators, sizeof,
    offsetof), in order: a program that prints them, compiled with gcc and run."""
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "jello_formats.h"\n#include "jello_hip.h"\nint main(void) {\n' + \
          "".join('    printf("%%lld\\n", (long long)(%s));\n' % e for e in expressions) + "    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "values.c"), os.path.join(d, "values")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", INCLUDE, c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert len(vals) == len(expressions)
    return vals
