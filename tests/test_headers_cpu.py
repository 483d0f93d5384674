"""Every header of csrc/ stands alone: it compiles on its own for gfx950 with the library's flags, so it includes what it uses and
depends on nothing that a translation unit happened to include before it."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from isingmontecarlo_amd import _build

HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(_build.CSRC, "*.h")))


def test_the_device_header_is_split():
    assert "sse_device.hip.h" not in HEADERS
    assert {"sse_batch.h", "sse_core.hip.h", "sse_diag.hip.h", "sse_unionfind.hip.h", "sse_cluster_pass.hip.h", "sse_loop.hip.h",
            "sse_sweep.hip.h", "sse_launch.h", "batch.hip.h", "lds_plan.h"} <= set(HEADERS)


def test_the_shared_data_header_is_plain_cpp():
    """sse_batch.h holds no device code: a host compiler without HIP takes it."""
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I.", "-x", "c++", "-"],
                       input='#include "sse_batch.h"\nstatic_assert(sizeof(sse::BondRec) == 16, "one dwordx4 load");\n',
                       cwd=_build.CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_the_tempering_rule_header_is_plain_cpp():
    """pt_rule.h is shared by the host, the decision kernel and a stand-alone test program: a host compiler without HIP takes it."""
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I.", "-x", "c++", "-"],
                       input='#include "pt_rule.h"\nbool f() { return pt_a_first(pt_chain(1, 2, 3), PtHostDraw{}) && pt_accept(1.0, 2.0, 3, 4, 1.0, 0.5); }\n',
                       cwd=_build.CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


KERNEL_HEADERS = {"sse_fast.hip.h", "sse_rvb.hip.h", "sse_rvb_split.hip.h", "sse_cluster.hip.h", "sse_sweep.hip.h",
                  "sse_diag.hip.h", "sse_cluster_pass.hip.h", "sse_unionfind.hip.h", "sse_loop.hip.h",  # these four: the passes behind sse_sweep.hip.h
                  "sse_classical.hip.h", "sse_classical_pt.hip.h", "sse_classical_overlap.hip.h", "sse_classical_icm.hip.h"}


def _includes(path, seen=None):
    """Every file of csrc/ that `path` includes, directly or through the headers it includes."""
    seen = set() if seen is None else seen
    with open(path) as f:
        for name in re.findall(r'^\s*#\s*include\s+"([^"/]+)"', f.read(), re.M):
            if name not in seen:
                seen.add(name)
                _includes(os.path.join(_build.CSRC, name), seen)
    return seen


def test_only_kernel_units_and_the_lds_plan_include_kernel_headers():
    """The host side of the C ABI (creation, driver, accessors, tempering, record) sees the kernels through sse_launch.h and lds_plan.h
    alone: no kernel header reaches it, not even through another header."""
    units = sorted(glob.glob(os.path.join(_build.CSRC, "*.hip")))
    assert {os.path.basename(u) for u in units} == set(_build.SOURCES)
    for unit in units:
        name = os.path.basename(unit)
        if name.startswith("sweep_") or name == "lds_plan.hip":
            continue
        assert not (_includes(unit) & KERNEL_HEADERS), (name, sorted(_includes(unit) & KERNEL_HEADERS))
    assert _includes(os.path.join(_build.CSRC, "lds_plan.hip")) & KERNEL_HEADERS  # (the walk does find them where they are)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    p = subprocess.run([hipcc] + _build.FLAGS + ["-Wno-pragma-once-outside-header", "-fsyntax-only", "-x", "hip", header],
                       cwd=_build.CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
