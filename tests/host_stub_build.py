"""The gcc command line of the CPU builds of the C host layer: build.HOST_SRC and
rfec_net.c against tests/host_stub/stub_hip.c (the host stand-in for the HIP
runtime and the kernel launches).  Shared by the tests that load such a build
(test_rx_shards.py, test_aux_kernels.py); the fixtures stay in the test files."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from razor_amd.build import HOST_SRC  # noqa: E402

ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
CSRC = ROOT / "razor_amd" / "csrc"
STUB = ROOT / "tests" / "host_stub"


def have_hip_headers() -> bool:
    return (ROCM / "include" / "hip" / "hip_runtime_api.h").exists()


def stub_cmd(out, flags=(), extra_src=()):
    """gcc: the host layer + the stub (+ extra_src, e.g. a main) -> out."""
    inc = [f"-I{ROCM / 'include'}", f"-I{ROOT / 'include'}", f"-I{CSRC}"]
    return ["gcc", "-std=c99", "-O1", "-g", *flags, "-DSIM_VIDEO_SIZE=1200", "-D__HIP_PLATFORM_AMD__", *inc,
            *(str(CSRC / f) for f in HOST_SRC), str(CSRC / "rfec_net.c"), str(STUB / "stub_hip.c"),
            *map(str, extra_src), "-o", str(out), "-lpthread", "-lm"]


def build_stub_library(out) -> Path:
    """The stub-linked host library (SIM_VIDEO_SIZE 1200) as a shared object at `out`."""
    r = subprocess.run(stub_cmd(out, flags=("-fPIC", "-shared")), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return Path(out)
