"""How the test tool tests/libnarrowphase_probe.so is built (tests/narrowphase_probe.hip: the device's narrow-phase templates behind a per-pair
entry).  Used by __graft_entry__.build() and, in a tree without the tool or with an older one, by tests/test_narrowphase_gpu.py."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "narrowphase_probe.hip")
LIBRARY = os.path.join(ROOT, "tests", "libnarrowphase_probe.so")


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
