"""How the test tool tests/libpair_distance_probe.so is built (tests/pair_distance_probe.hip: the per-pair distance routine of
furniture_amd/csrc/fsim_gjk.hpp behind a per-case entry).  Used by __graft_entry__.build() and, in a tree without the tool or with an older
one, by tests/test_pairs_tool_gpu.py."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "pair_distance_probe.hip")
LIBRARY = os.path.join(ROOT, "tests", "libpair_distance_probe.so")


def probe_command(so=LIBRARY):
    """the library's own hipcc line (furniture_amd.sim.hipcc_command: same optimisation and floating-point flags) with the tool's source"""
    from furniture_amd import sim
    cmd = sim.hipcc_command(so)
    assert cmd[-3] == "-o" and cmd[-1].endswith("fsim.hip"), cmd
    return cmd[:-1] + [SOURCE]


def stale():
    csrc = os.path.join(ROOT, "furniture_amd", "csrc")
    deps = [SOURCE] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    return not os.path.exists(LIBRARY) or any(os.path.getmtime(d) > os.path.getmtime(LIBRARY) for d in deps)
