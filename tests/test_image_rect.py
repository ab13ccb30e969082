"""The geometry the image calls share (include/jello_image.h) and the scratch sizes of the blur and resample rules, on the CPU: the
stand-alone check tools/image_rect_check.cpp."""
import os
import shutil
import subprocess

import pytest

from abi_text import INCLUDE, ROOT


def test_the_stand_alone_check_builds_and_passes(tmp_path):
    """tools/image_rect_check.cpp is include/jello_image.h, jello_blur.h and jello_resample.h with a main of its own: the row window
    and the blur's scratch size against a brute-force count of rows and against the formula jh_blur had of its own, the resample's
    scratch size, and the rectangle check's three answers up to the 32-bit limits.  Its header has the command with the sanitizers;
    here it is built without them and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "image_rect_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", INCLUDE, os.path.join(ROOT, "tools", "image_rect_check.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode() == "ok\n"
