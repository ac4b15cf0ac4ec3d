"""-m gpu: the host pipeline of spl_encode_batch under ThreadSanitizer (VERDICT r02 missing #6).
tools/build_sanitizers.sh rebuilds the library's host side with -fsanitize=thread (the device code is unchanged) and
tests/san/hostpath_driver.cpp, which drives a two-pipeline handle and a custom-pattern handle (host splitter
threads) from two caller threads at once in many small chunks and checks every result.  Frames inside the
uninstrumented HIP / HSA runtimes are suppressed (tests/san/tsan.supp); anything in this repo's code is reported.

ThreadSanitizer's x86-64 address map is fixed at compile time: application memory may lie only in the three windows
of _TSAN_APP below, everything between them is shadow or is sealed off when the program starts.  The HSA runtime in
turn accepts a mapping only inside the range the GPU driver can address.  Where a driver confines that range to
addresses between ThreadSanitizer's windows (a GPU reached through a proxy driver does: every mapping made after the
device is opened lands below 0x5000'0000'0000, the device's own included), no address satisfies both, the runtime
under ThreadSanitizer cannot map anything and reports that there is no device.  The test reads where this process's
own HIP runtime mapped the device and skips itself, with that as the reason, when ThreadSanitizer could not hold it."""
import os
import platform
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
B = os.path.join(ROOT, "tests", "san", "_build")
DATA = os.path.join(ROOT, "splintr_amd", "data")

# compiler-rt, tsan_platform.h, Mapping48AddressSpace (C/C++, linux/x86_64): low, middle and high application memory
_TSAN_APP = ((0x000000001000, 0x020000000000), (0x550000000000, 0x5a0000000000), (0x7a0000000000, 0x800000000000))


def _device_mappings_outside_tsan_app():
    """The start addresses of this process's /dev/kfd and /dev/dri/renderD* mappings that ThreadSanitizer's address map
    has no room for (an empty list: all of them fit, or the map is not the x86-64 one)."""
    if platform.machine() != "x86_64":
        return []
    from splintr_amd import _ffi
    assert _ffi.lib().spl_device_count() >= 1                    # the HIP runtime is up: the device is opened and mapped
    bad = []
    with open("/proc/self/maps") as f:
        for line in f:
            m = re.match(r"([0-9a-f]+)-([0-9a-f]+) .*(/dev/kfd|/dev/dri/renderD\d+)$", line.rstrip())
            if m:
                lo, hi = int(m.group(1), 16), int(m.group(2), 16)
                if not any(a <= lo and hi <= b for a, b in _TSAN_APP):
                    bad.append(lo)
    return bad


def test_host_pipeline_under_thread_sanitizer():
    bad = _device_mappings_outside_tsan_app()
    if bad:
        pytest.skip(f"the GPU driver here maps the device at {min(bad):#x}..{max(bad):#x}, addresses that ThreadSanitizer's "
                    "fixed address map keeps for its shadow: the HIP runtime cannot come up under ThreadSanitizer")
    exe = os.path.join(B, "hostpath_tsan")
    # the script decides staleness by a hash of the sources: a library built from an older tree is rebuilt, not run
    subprocess.check_call([os.path.join(ROOT, "tools", "build_sanitizers.sh")], timeout=1500, stdout=subprocess.DEVNULL)
    env = dict(os.environ, TSAN_OPTIONS=f"suppressions={os.path.join(ROOT, 'tests', 'san', 'tsan.supp')} halt_on_error=0 report_signal_unsafe=0")
    p = subprocess.run([exe, os.path.join(DATA, "cl100k_base.splv"), os.path.join(DATA, "unicode_classes.bin")],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-4000:])
    assert "consistent" in p.stdout
    ours = [blk for blk in p.stderr.split("==================") if "WARNING: ThreadSanitizer" in blk
            and ("spl_" in blk or "splintr" in blk or "hostpath_driver" in blk)]
    assert not ours, ours[0][-4000:]
