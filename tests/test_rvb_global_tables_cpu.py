"""CPU-side checks of the RVB-with-tables-in-HBM switch (ISINGMC_CFG_RVB_GLOBAL_TABLES): the Python mirror of the flag and of its
launch_info bit agree with the public header, and the flag is a distinct bit."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_defines():
    text = open(os.path.join(ROOT, "include", "isingmc_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (ISINGMC_CFG_\w+) (\d+)u", text)}


def test_flag_mirrors_the_header_and_is_exported():
    import isingmontecarlo_amd as im
    d = header_defines()
    assert d["ISINGMC_CFG_RVB_GLOBAL_TABLES"] == im.CFG_RVB_GLOBAL_TABLES == 4096
    assert "CFG_RVB_GLOBAL_TABLES" in im.__all__
    others = [v for k, v in d.items() if k != "ISINGMC_CFG_RVB_GLOBAL_TABLES"]
    assert all(v & im.CFG_RVB_GLOBAL_TABLES == 0 for v in others), d  # a bit of its own
    for k, v in d.items():  # every flag the header defines has its Python mirror with the same value
        assert getattr(im, k[len("ISINGMC_"):]) == v, k


def test_launch_info_documents_the_bit():
    text = open(os.path.join(ROOT, "include", "isingmc_hip.h")).read()
    assert re.search(r"bit 7: the most recent RVB sweep kept its per-variable\s+\*\s+tables in HBM", text)
    src = open(os.path.join(ROOT, "isingmontecarlo_amd", "__init__.py")).read()
    assert "rvb_global_tables=bool(out[6] & 128)" in src
