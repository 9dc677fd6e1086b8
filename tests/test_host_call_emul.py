"""CPU check of the host-pointer forms' staging scope (lachain_amd/csrc/host_call.hpp: HostCall, rebase) compiled by
tools/emul/host_call_emul.cpp against a stand-in HIP runtime (tools/emul/hip_stub) whose device memory is the heap at
its exact size: a stand-alone program built with -fsanitize=address,undefined.  Its cases: slots in request order whose
contents round-trip, a zero count, reuse across calls (slots grow, never shrink), an allocation failure at every
position, one request beyond the slot count, a nested call behind the outer one's slots, wipe's clamp, and the offset
rebase.  It must exit 0 and leave no sanitizer report.  TEST INFRASTRUCTURE: the entry points that use the scope are
covered on the GPU by tests/test_gpu_host_forms_interleaved.py and the feature tests."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "host_call_emul.cpp")
EXE = os.path.join(ROOT, "tools", "emul", "host_call_emul")
STUB = os.path.join(ROOT, "tools", "emul", "hip_stub")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC, os.path.join(STUB, "hip", "hip_runtime.h")] + [
    os.path.join(CSRC, f) for f in ("host_call.hpp", "lcb_ctx.hpp", "lcb_internal.hpp")]


def test_host_call_emul():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread", "-I", STUB,
                        "-o", EXE, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([EXE], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert "host_call_emul: ok" in out.stdout
