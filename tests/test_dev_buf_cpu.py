"""DevBuf (opt_amd/csrc/dev_buf.h), the self-freeing device buffer of the graph kernel sets, as plain C++: tests/dev_buf_driver.cpp counts allocations and frees through
stand-ins for hipMalloc / hipFree and runs under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "opt_amd", "csrc")


def test_every_allocation_is_freed_exactly_once(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    exe = str(tmp_path / "dev_buf_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                           os.path.join(HERE, "dev_buf_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 5", (r.returncode, r.stdout, r.stderr[-3000:])
