"""What tests/test_weak_hash_cpu.py, tests/test_gpu_weak_hash.py and the weak-hash tests of
tests/test_gpu_cache.py and tests/test_gpu_fused_vgreedy.py share: where the variant library is, how a job is handed to tests/weak_hash_child.py, and the key packer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

VARIANT = os.path.join(PKG_ROOT, "acx", "libacx_weakhash.so")
CHILD = os.path.join(REPO, "tests", "weak_hash_child.py")
CLASSES = 8
FATAL = (124, 134, 139)  # a time limit, an abort, a segmentation fault; a negative code is the signal that ended the child


def variant():
    assert os.path.exists(VARIANT), (f"{VARIANT} is missing: build it with `python ac-solver-caltech_amd/build.py` "
                                     "(it makes libacx.so and the weak-hash variant)")
    return VARIANT


class ChildDied(Exception):
    pass


def run_child(calls, workdir, timeout):
    """The calls, made in one fresh process under ACX_LIB=<variant> -> (their answers, the arrays
    they returned, the child's wall time in seconds).  ChildDied: the child ended on a signal, an
    abort or its timeout."""
    import time
    workdir = str(workdir)
    with open(os.path.join(workdir, "in.json"), "w") as f:
        json.dump({"calls": calls}, f)
    env = dict(os.environ, ACX_LIB=variant())
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, CHILD, workdir], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        raise ChildDied(f"timeout after {timeout} s: {str(e.stderr)[-2000:]}") from None
    dt = time.perf_counter() - t0
    if r.returncode < 0 or r.returncode in FATAL:
        raise ChildDied(f"exit code {r.returncode}: {r.stderr[-2000:]}")
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])["results"]
    assert len(out) == len(calls)
    with np.load(os.path.join(workdir, "out.npz")) as z:
        arrays = {k: z[k] for k in z.files}
    return out, arrays, dt


def pack_keys_np(states, L):
    """(n, 2L) presentations -> (n, kw) packed keys (csrc/acx_key.h: 2-bit letter codes of r0 then
    r1 from bit 0, the two lengths in a byte each from bit 4L); conftest.unpack_keys_np's inverse"""
    states = np.asarray(states, np.int64)
    n, kw = states.shape[0], (4 * L + 16 + 63) // 64
    bits = np.zeros((n, kw * 64), np.uint8)
    code = np.zeros(5, np.uint8)
    code[[1 + 2, -1 + 2, 2 + 2, -2 + 2]] = [0, 1, 2, 3]
    c = code[states + 2] * (states != 0)
    bits[:, 0:4 * L:2] = c & 1
    bits[:, 1:4 * L:2] = c >> 1
    for h in range(2):
        ln = (states[:, h * L:(h + 1) * L] != 0).sum(1)
        for j in range(8):
            bits[:, 4 * L + 8 * h + j] = (ln >> j) & 1
    return np.packbits(bits.reshape(n, kw, 64), axis=2, bitorder="little").view("<u8").reshape(n, kw)


def check_classes(nodes, classes, what):
    """the non-vacuity bound of a job: its nodes fall in at most 8 hash classes of at least 64 nodes
    on average, so (pigeonhole) every insert met entries of other states with its fingerprint"""
    assert 1 <= classes <= CLASSES and nodes >= 64 * classes, (what, nodes, classes)


def skip_after_death(dead):
    if dead:
        pytest.skip(f"an earlier weak-hash child died ({dead[0]}): nothing more is started on the card")
