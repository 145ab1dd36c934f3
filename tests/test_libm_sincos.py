"""The fused sincosf of the device code (one range reduction for both results) against the running glibc's sinf and cosf, on every
float of [0, 7]: the domain test_abi_cpu.py checks sinf_glibc and cosf_glibc on, and wider than the [0, 2 pi] the path produces."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SINCOS_CHECK = r"""
#include <cmath>
#include <cstdio>
#include "%s"
int main() {
    unsigned long n = 0, bad = 0;
    for(uint32_t u = 0; u <= ptm::as_u32(7.0f); u++, n++) {
        const float f = ptm::as_f32(u);
        float s, c;
        ptm::sincosf_glibc(f, &s, &c);
        bad += ptm::as_u32(sinf(f)) != ptm::as_u32(s);
        bad += ptm::as_u32(cosf(f)) != ptm::as_u32(c);
    }
    printf("%%lu %%lu\n", n, bad);
    return 0;
}
"""


def test_sincosf_matches_glibc_sinf_cosf(tmp_path):
    src = tmp_path / "sincos_check.cpp"
    src.write_text(SINCOS_CHECK % os.path.join(ROOT, "cpupathtrace_amd", "csrc", "pt_libm.h"))
    exe = tmp_path / "sincos_check"
    subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-o", str(exe), str(src)], check=True)
    n, bad = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(n) == 0x40E00000 + 1 and int(bad) == 0
