"""The two weight packers of csrc/rn_pack.h (through tools/pack_main.cpp, a host program) against a NumPy restatement of the layout
formulas in the comments over them, byte for byte.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BF16, F16 = 1, 2          # RN_DTYPE_*

# (chunks of 32 K elements, couts) of the five kernels that take the K32 layout
K32_CASES = {"stage4x": (9, 64), "stage5x": (18, 64), "stage6x": (18, 128), "conv16": (18, 128), "conv16p": (36, 16)}


@pytest.fixture(scope="module")
def pack_main(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pack") / "pack_main")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "roomnet_amd", "csrc"), os.path.join(ROOT, "tools", "pack_main.cpp"), "-o", exe])
    return exe


def kernel(k, cout, seed):
    """A seeded random [k][cout] kernel; every tenth entry or so is a value at which a 16-bit conversion can go wrong."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((k, cout)) * 0.1).astype(np.float32)
    special = np.array([
        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,      # exact ties of fp16 / bf16 (to even: down, up)
        0.1 + 2.0 ** -15, 2.0 ** -14 - 2.0 ** -25,                                 # ... and a tie that carries into the next binade
        2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 3e-6, 6.0e-5, 2.0 ** -26,        # fp16 subnormals, ties among them, underflow
        65504.0, 65519.0, 65520.0, 70000.0, 1e6, 3e38,                             # fp16's largest, the last below the tie, overflow
        0.0, 1.0 / 6.0,
    ], np.float32)
    at = rng.random((k, cout)) < 0.1
    w[at] = rng.choice(special, int(at.sum())) * rng.choice(np.array([-1, 1], np.float32), int(at.sum()))
    return w


def to16(w, dtype):
    """float32 -> the 16-bit storage type's bits, round to nearest, ties to even (finite inputs)"""
    if dtype == F16:
        with np.errstate(over="ignore"):
            return w.astype(np.float16).view(np.uint16)
    u = w.view(np.uint32)
    kept, dropped = u >> 16, u & 0xFFFF
    up = (dropped > 0x8000) | ((dropped == 0x8000) & (kept & 1 == 1))
    return (kept + up).astype(np.uint16)


def run(exe, tmp_path, args, w):
    src, dst = str(tmp_path / "w.bin"), str(tmp_path / "frag.bin")
    w.tofile(src)
    subprocess.check_call([exe] + [str(a) for a in args] + [src, dst])
    return np.fromfile(dst, np.uint16)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("family", sorted(K32_CASES))
def test_k32_fragments(pack_main, tmp_path, family, dtype):
    """frag[chunk c][cout tile t][lane][j] = W[32 c + 8 (lane / 16) + j][16 t + lane % 16]"""
    nchunks, cout = K32_CASES[family]
    w = kernel(32 * nchunks, cout, seed=nchunks * 1000 + cout)
    got = run(pack_main, tmp_path, ["k32", nchunks, cout, dtype], w)
    c, t, lane, j = np.ogrid[:nchunks, :cout // 16, :64, :8]
    want = to16(w, dtype)[32 * c + 8 * (lane // 16) + j, 16 * t + lane % 16]
    assert got.size == want.size
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    assert len(np.unique(want)) > 1000          # (the kernel is not degenerate)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cout", [64, 128])
def test_k48_fragments(pack_main, tmp_path, cout, dtype):
    """frag[ky * 5 + j][cout tile t][lane][e], g = lane / 16: j < 3: W[tap (ky, j)][8 g + e]; j = 3: groups 0, 1 = W[tap (ky, 0)][32 + 8 g + e],
    groups 2, 3 = W[tap (ky, 1)][32 + 8 (g - 2) + e]; j = 4: groups 0, 1 = W[tap (ky, 2)][32 + 8 g + e], groups 2, 3 = 0"""
    w = kernel(9 * 64, cout, seed=48000 + cout)
    got = run(pack_main, tmp_path, ["k48", cout, dtype], w).reshape(3, 5, cout // 16, 4, 16, 8)      # [ky][j][t][g][lane % 16][e]
    w16 = to16(w, dtype).reshape(3, 3, 64, cout // 16, 16)                                              # [ky][kx][channel][t][cout % 16]
    want = np.zeros_like(got)
    for ky in range(3):
        for g in range(4):
            chan = lambda kx, first: w16[ky, kx, first:first + 8].transpose(1, 2, 0)                    # [t][cout % 16][e]
            for j in range(3):
                want[ky, j, :, g] = chan(j, 8 * g)
            want[ky, 3, :, g] = chan(0, 32 + 8 * g) if g < 2 else chan(1, 32 + 8 * (g - 2))
            if g < 2:
                want[ky, 4, :, g] = chan(2, 32 + 8 * g)
    np.testing.assert_array_equal(got, want)
    assert not got[:, 4, :, 2:].any()           # what the kernels multiply with the lanes that re-read tap column 2: zero weights
    assert got[:, 4, :, :2].any() and got[:, 3, :, 2:].any()
