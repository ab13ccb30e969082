"""CPU: libjello_hip.so loads without a GPU and exports every symbol include/jello_hip.h declares; the ctypes mirrors of the
header's structs have the header's layout and every call engine.py makes on the C ABI is declared; without a device the engine
fails loudly (no fallback)."""
import ctypes
import inspect
import os
import re

import pytest

import jello_amd
from jello_amd import _lib

from abi_text import c_values, header_arity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "jello_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(jh_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_are_exported(built):
    lib = ctypes.CDLL(jello_amd.lib_paths()["hip"])
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), "missing export: " + s


def test_stage_enum_matches_fullshaders_order(built):
    lib = ctypes.CDLL(jello_amd.lib_paths()["hip"])
    lib.jh_stage_name.restype = ctypes.c_char_p
    names = [lib.jh_stage_name(i).decode() for i in range(22)]
    assert names == jello_amd.STAGE_NAMES  # renderer/render.go:17-43


def test_formats_header_sizes():
    """include/jello_formats.h carries static_asserts; compile it as C and C++."""
    import subprocess
    import tempfile
    for comp, ext in (("gcc", "c"), ("g++", "cpp")):
        with tempfile.NamedTemporaryFile("w", suffix="." + ext, delete=False) as f:
            f.write('#include "jello_formats.h"\n#include "jello_hip.h"\nint main(void){return sizeof(JlConfig)==100?0:1;}\n')
        out = f.name + ".bin"
        subprocess.check_call([comp, "-I", os.path.join(ROOT, "include"), f.name, "-o", out])
        assert subprocess.call([out]) == 0
        os.unlink(f.name)
        os.unlink(out)


MIRRORS = {"jh_yuv_desc": _lib.CYuvDesc, "jh_blur_desc": _lib.CBlurDesc, "jh_composite_desc": _lib.CCompositeDesc,
           "jh_dash_path": _lib.CDashPath, "jh_dash_el": _lib.PathEl, "jh_profile_record": _lib.CProfileRecord,
           "jh_profile_node": _lib.CProfileNode}


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_ctypes_mirror_has_the_headers_layout(struct):
    """sizeof and the offsetof of every field, as the compiled header states them."""
    mirror = MIRRORS[struct]
    fields = [name for name, _ in mirror._fields_]
    want = c_values(["sizeof(%s)" % struct] + ["offsetof(%s, %s)" % (struct, f) for f in fields])
    assert [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields] == want, (struct, fields, want)


def test_image_format_enum_matches_header():
    from jello_amd import ImageFormat
    names = [f.name for f in ImageFormat]
    assert names == ["RGBA8", "RGBA8_SRGB", "BGRA8", "RGBA16_FLOAT"]
    assert c_values(["JL_" + n for n in names]) == [int(f) for f in ImageFormat] == [0, 1, 2, 3]


def test_every_call_engine_py_makes_on_the_c_abi_is_declared(built):
    """Engine calls the C ABI through ctypes directly: a call without argtypes would pass 64-bit ids and pointers as C ints."""
    with open(os.path.join(ROOT, "jello_amd", "engine.py")) as f:
        called = sorted(set(re.findall(r"\bhip\.(jh_\w+)\(", f.read())))
    assert len(called) > 30 and {"jh_blit", "jh_blit_yuv", "jh_pack_tiles", "jh_unpack_tiles", "jh_dash", "jh_blur", "jh_composite",
                                 "jh_image_upload", "jh_image_create", "jh_image_free"} <= set(called)
    declared = dict(re.findall(r"\bhip\.(jh_\w+)\.argtypes = \[(.*)", inspect.getsource(_lib._declare)))
    arity, hip = header_arity(), jello_amd.load_host().hip
    for name in called:
        assert name in declared, "engine.py calls hip.%s, which _lib._declare gives no argtypes" % name
        assert len(getattr(hip, name).argtypes) == arity.get(name), "hip.%s: argtypes differ in length from the header's declaration" % name


def test_no_gpu_means_loud_failure(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        jello_amd.Engine(0)
