"""Memory safety of the split JPEG decoder's two entry points and the host pixel stage: tools/fuzz_jpeg_split.c and
bcnn_amd/host/bip_jpeg.c compiled into one stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(CPU build, a process of its own). It feeds every fixture of tests/golden/jpeg, its truncations at every 37th byte and 400
single-byte corruptions per file (fixed seed) through bip_jpeg_frame_info / bip_jpeg_read_coefficients /
bip_jpeg_pixels_from_coefficients with heap buffers of exactly the advertised sizes, and checks the result against the
one-call decoder."""
import os
import subprocess

from tests import _jpeg_fixtures as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixtures_truncations_and_corruptions_never_trip_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fuzz_jpeg_split")
    cmd = ["gcc", "-std=gnu99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bcnn_amd", "host"),
           os.path.join(ROOT, "tools", "fuzz_jpeg_split.c"), os.path.join(ROOT, "bcnn_amd", "host", "bip_jpeg.c"),
           "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [os.path.join(J.DIR, n) for n in J.NAMES], capture_output=True, text=True, env=env,
                       timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "runtime error" not in tail and "AddressSanitizer" not in tail and "LeakSanitizer" not in tail, tail
    streams, decoded = (int(x) for x in r.stdout.split()[0:3:2])
    assert streams > 400 * len(J.NAMES) and decoded >= len(J.NAMES), r.stdout
