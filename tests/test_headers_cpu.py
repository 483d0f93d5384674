"""Every header of csrc/ stands alone: it compiles on its own for gfx950 with the library's flags, so it includes what it uses and
depends on nothing that a translation unit happened to include before it."""
import glob
import os
import shutil
import subprocess

import pytest

from isingmontecarlo_amd import _build

HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(_build.CSRC, "*.h")))


def test_the_device_header_is_split():
    assert "sse_device.hip.h" not in HEADERS
    assert {"sse_batch.h", "sse_core.hip.h", "sse_diag.hip.h", "sse_unionfind.hip.h", "sse_cluster_pass.hip.h", "sse_loop.hip.h",
            "sse_sweep.hip.h", "sse_launch.h", "batch.hip.h"} <= set(HEADERS)


def test_the_shared_data_header_is_plain_cpp():
    """sse_batch.h holds no device code: a host compiler without HIP takes it."""
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I.", "-x", "c++", "-"],
                       input='#include "sse_batch.h"\nstatic_assert(sizeof(sse::BondRec) == 16, "one dwordx4 load");\n',
                       cwd=_build.CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    p = subprocess.run([hipcc] + _build.FLAGS + ["-Wno-pragma-once-outside-header", "-fsyntax-only", "-x", "hip", header],
                       cwd=_build.CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
