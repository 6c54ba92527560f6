"""csrc/per_device.h on the host: tests/per_device_main.cpp (its own main, includes only that header) built with the host g++
plain, under the thread sanitizer and under the address + undefined-behaviour sanitizers; each binary is run as a program of its
own (nothing is preloaded, nothing loaded into python is sanitised).  The program checks: 8 threads x 1000 gets over 4 ordinals
see one value per slot, a failed init is retried and not cached, ordinals -1 and 64 are never cached, two objects share nothing."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "per_device_main.cpp")
INC = os.path.join(ROOT, "m3dssd_amd", "csrc")
_LIBC = ctypes.CDLL(None)


def _fixed_address_space():
    """In the child, before exec: personality(ADDR_NO_RANDOMIZE) for this one process.  gcc's thread sanitizer refuses to start
    ("unexpected memory mapping") where the kernel randomises mappings over more bits than its shadow layout allows for; newer
    runtimes re-exec themselves this way.  Where the call is not permitted the program starts as it is."""
    _LIBC.personality(0x0040000)


# (the sanitizer runtimes are linked statically: the binary then runs whatever else the environment loads into a process)
@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread", "-static-libtsan"],
                                   ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]],
                         ids=["plain", "tsan", "asan_ubsan"])
def test_per_device_program(flags, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no host g++")
    exe = str(tmp_path / "per_device_main")
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", INC] + flags + [SRC, "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, preexec_fn=_fixed_address_space)
    assert run.returncode == 0 and "PER_DEVICE_OK" in run.stdout, run.stdout[-4000:]
