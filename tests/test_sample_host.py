"""CPU checks of the samplers' boundary: the Python restatement of the generator (include/gvi_hip.h, "samples of q")
reproduces the Random123 Philox4x32-10 known answers, and GVIGH::sample / GVIGH::log_density compile against the shim."""
import math
import os
import subprocess

import numpy as np

from gaussianvi_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
    return c0, c1, c2, c3


def randn(seed, first, count):
    """Normal numbers first .. first + count - 1 of stream `seed`: the generator gvi_randn / gvi_bt_sample use."""
    out = np.empty(count)
    key = (seed & M32, (seed >> 32) & M32)
    for i in range(first, first + count):
        c = i >> 1
        w = philox4x32_10((c & M32, (c >> 32) & M32, 0, 0), key)
        u1 = (((w[0] | w[1] << 32) >> 11) + 0.5) * 2.0 ** -53
        u2 = (((w[2] | w[3] << 32) >> 11) + 0.5) * 2.0 ** -53
        r = math.sqrt(-2.0 * math.log(u1))
        out[i - first] = r * (math.cos(2 * math.pi * u2) if i % 2 == 0 else math.sin(2 * math.pi * u2))
    return out


def test_philox_known_answers():
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_restated_generator_is_split_invariant_and_standard():
    z = randn(7, 3, 4000)
    assert np.array_equal(z[10:20], randn(7, 13, 10))           # number i depends on (seed, i) only
    assert not np.array_equal(z[:100], randn(8, 3, 100))
    assert abs(z.mean()) < 6 / math.sqrt(len(z)) and abs(z.var() - 1.0) < 6 * math.sqrt(2.0 / len(z))


def test_sample_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "sample_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "sample_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
