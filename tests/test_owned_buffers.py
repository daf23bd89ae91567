"""The owners of GPU resources (csrc/owned.h) free what they made exactly once, and a size lives with its pointer.

The header is host-only C++ over <hip/hip_runtime_api.h>, so tests/stub/owned_fake_hip.cpp compiles it with g++ against its own
counting definitions of the few runtime calls the header makes, links no HIP library and runs under AddressSanitizer and
UndefinedBehaviorSanitizer as an ordinary program.  What it asserts is in its source: nothing alive after scope exit, reset,
moves (self-moves included), adopt and release; what grow calls and leaves behind; for each group the engine makes on first use
(pinned staging, overlap-save side stream, kernel timing) a failure at every one of its creations, then a clean retry; and the
group driver's capacity, which reads 0 after a failure at any rank."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "owned_fake_hip")
    src = os.path.join(ROOT, "tests", "stub", "owned_fake_hip.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing of them is looked up when it starts)
                         "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout.decode(errors="replace")[-1500:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout.decode(errors="replace")[-400:], p.stderr.decode(errors="replace")[-1500:])
    word = p.stdout.decode().split()
    assert word[0] == "ok" and int(word[1]) > 1000
