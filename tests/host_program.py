"""Build one of the stand-alone programs under tests/host/ with ASan + UBSan and run it as a process of its own.

The programs include a host-only header of csrc/ (the plan headers) and tests/host/check.h; no sanitizer runtime is ever loaded into the
test process.  A helper module like tests/guarded.py: no tests are collected from it."""
import os
import shutil
import subprocess

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")


def host_compilers():
    """[(compiler, extra flags)] of every distinct host C++ compiler here: the sanitizer runtimes linked statically (clang's default), so
    that the program starts whatever the environment preloads into every process."""
    found, seen = [], set()
    for cxx, extra in (("/opt/rocm/llvm/bin/clang++", []), ("clang++", []), ("g++", ["-static-libasan", "-static-libubsan"])):
        path = shutil.which(cxx)
        if path and os.path.realpath(path) not in seen:
            seen.add(os.path.realpath(path))
            found.append((path, extra))
    return found


def run_alone_under_sanitizers(cpp_name, tmp_path):
    """{compiler: stdout lines} of tests/host/<cpp_name> built by every host compiler found.  Asserts for each: exit status 0, no line
    starting FAILED, nothing on stderr (a sanitizer report goes there), and the closing line of check.h."""
    compilers = host_compilers()
    assert compilers, "no host C++ compiler: the library was built here, so one exists"
    out = {}
    for k, (cxx, extra) in enumerate(compilers):
        exe = tmp_path / f"{os.path.splitext(cpp_name)[0]}_{k}"
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra,
                        os.path.join(HOST, cpp_name), "-o", str(exe)], check=True)
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        lines = run.stdout.splitlines()
        failed = [ln for ln in lines if ln.startswith("FAILED")]
        assert run.returncode == 0 and not failed and not run.stderr, cxx + "\n" + "\n".join(failed[:20]) + "\n" + run.stderr[-4000:]
        assert lines[-1] == "ok: 0 failed checks", cxx
        out[cxx] = lines
    return out
