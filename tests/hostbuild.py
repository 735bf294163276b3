"""How the host-code tests (tests/test_*_host.py) build their tests/*_host/*.hip sources: as a shared object for ctypes, and as a
stand-alone program with its own main under AddressSanitizer / UBSan (host part only).  Nothing is loaded into Python under a
sanitizer and nothing here runs on a GPU."""
import os
import shutil
import subprocess

SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def hipcc():
    cc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    assert cc, "hipcc is what builds this project"
    return cc


def shared(src, tmpdir):
    """the path of lib<name>.so built from `src` in tmpdir"""
    so = os.path.join(str(tmpdir), "lib" + os.path.splitext(os.path.basename(src))[0] + ".so")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", src, "-o", so])
    return so


def sanitized_run(src, define, tmp_path):
    """`src` with -D<define> (its own main) under AddressSanitizer / UBSan: built, run once, and clean — no sanitizer report, exit
    status 0, nothing on stderr, and the program's own count of failures 0.  Returns its stdout."""
    probe = tmp_path / "probe.hip"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([hipcc(), "--offload-arch=gfx950", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    assert r.returncode == 0, "hipcc cannot link the AddressSanitizer / UBSan runtime: the check cannot run\n" + r.stderr[-2000:]
    exe = tmp_path / (define.lower() + "_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-D" + define, *SAN, src, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[:4000]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[:2000])
    assert r.stderr.strip() == "", r.stderr[:2000]
    assert " 0 failures" in r.stdout
    return r.stdout
