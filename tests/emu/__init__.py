"""TEST INFRASTRUCTURE ONLY: builds (on demand) and loads the CPU-emulated build of the HIP
kernel sources (see tests/emu/include/hip/hip_runtime.h) and injects it into the package loader."""
import ctypes
import fcntl
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EMU_LIB = os.path.join(HERE, "liblbc_emu.so")


def build():
    # one make at a time: pytest-xdist workers on a clean tree would otherwise link the library under each other's feet
    with open(EMU_LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "learningbycheating_amd", "csrc"), "emu"])
    return EMU_LIB


def activate():
    from learningbycheating_amd import _lib
    build()
    return _lib._inject_for_tests(ctypes.CDLL(EMU_LIB))


def deactivate():
    from learningbycheating_amd import _lib
    _lib._inject_for_tests(None)
