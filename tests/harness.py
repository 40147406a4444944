"""The host harnesses of tests/*.cpp (the kernel header csrc/gs_device_math.h compiled for the CPU): the one place that says how they are built.
-ffp-contract=off decides bits in every model that is held against one of them."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FP = ["-ffp-contract=off", "-fno-fast-math"]
FLAGS = ["-std=c++17"] + FP
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]      # the stand-alone *_HARNESS_MAIN programs


def build_harness(dirpath, source, flags=FLAGS, defines=(), exe=False) -> str:
    """g++ over tests/<source> into dirpath: a shared library (-O2 unless the flags set a level), or with exe=True a program; returns its path"""
    name = os.path.splitext(source)[0]
    out = os.path.join(str(dirpath), name if exe else f"lib{name}.so")
    opt = [] if any(f.startswith("-O") for f in flags) else ["-O2"]
    subprocess.check_call(["g++"] + opt + ([] if exe else ["-fPIC", "-shared"]) + list(flags) + [f"-D{d}" for d in defines] + ["-o", out, os.path.join(HERE, source)])
    return out


def run_under_sanitizers(dirpath, source, define) -> subprocess.CompletedProcess:
    """the harness as a stand-alone program (its own main under `define`), built with the host sanitizers and run as a child process"""
    exe = build_harness(dirpath, source, SANITIZE + FLAGS, [define], exe=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


_host_math = None


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    """tests/host_math_harness.cpp, built once per session; a test module that uses it imports it by name"""
    global _host_math
    if _host_math is None:
        lib = C.CDLL(build_harness(tmp_path_factory.mktemp("hm"), "host_math_harness.cpp"))
        lib.hm_f16tof32.restype = C.c_float
        lib.hm_f16tof32.argtypes = [C.c_uint32]
        lib.hm_f32tof16.restype = C.c_uint32
        lib.hm_f32tof16.argtypes = [C.c_float]
        _host_math = lib
    return _host_math
