"""The owning handles of the host layer (csrc/gs_handles.h) against a fake HIP runtime that tracks every live allocation and event.

tests/handles_harness.cpp is a stand-alone program: it defines the few hip* functions the header calls, so it needs no GPU and no HIP runtime,
and it is built with AddressSanitizer + UBSan.  It exits non-zero on a double release, a leak, a handle that is not null after a failed
allocation, or a set of buffers that changed although its growth failed.

The fake runtime also has streams with vector clocks (an event snapshots its stream's clock at a record, a wait merges the snapshot of that moment), and
aborts if an event is ever recorded on a second stream.  Against it the harness checks gs::order_after -- work on the signaller before the call
happens-before work on the waiter after it, work put on the signaller afterwards does not -- and the sequences the library builds from it: the mirror
of a bit buffer into two lanes (owner's write -> each lane's copy -> owner's next write; a frame dealt earlier stays before its lane's copy), the
bracket of a move (lanes' earlier frames -> kernel -> lanes' later frames), and re-recording (an earlier wait keeps the snapshot of its own record)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    raise FileNotFoundError("hip/hip_runtime_api.h (set ROCM_PATH)")


def test_handles_under_sanitizers(tmp_path):
    exe = str(tmp_path / "handles_harness")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I" + rocm_include(), "-o", exe, os.path.join(HERE, "handles_harness.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "handles ok" in p.stdout and "ordering ok" in p.stdout
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr
