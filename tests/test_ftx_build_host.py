"""The FilteredTransaction builder on the CPU: cg_ftx_build_layout (a pure host function of
libcordagpu) and the host build of the device logic (cg_pmt_build.h, the exact per-tx pass
the HIP kernel compiles; tests/native/cg_ftxbuild_host.cpp) against the oracle's restatement
(oracle/py/merkle_tx.py) on every (component count, include mask) up to 10 components; the
same code as a stand-alone program under ASan + UBSan (tests/native/ftxbuild_san.cpp); the
plain-C and JNI callers without a device.  No GPU.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import ftx_build_util as U
from corda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
INCLUDE = ["-I", os.path.join(ROOT, "include")]
LINK = ["-L", os.path.join(ROOT, "corda_amd"), "-lcordagpu", "-Wl,-rpath,$ORIGIN/../../corda_amd",
        "-Wl,-rpath,/opt/rocm/lib"]


@pytest.fixture(scope="module")
def exhaustive():
    b = U.Batch(U.exhaustive_txs())
    return b, U.oracle_batch(b)


@pytest.fixture(scope="module")
def big():
    """k = 257 and k = 1,000 with sparse and dense masks, a transaction without components."""
    rng = np.random.default_rng(1000)
    shapes = [(257, [5]), (257, range(256)), (257, [255]), (1000, [0, 517, 998]), (1000, range(0, 999, 2)),
              (1000, range(999))]
    txs = []
    for k, idx in shapes:
        m = [0] * k
        for i in idx:
            m[i] = 1
        txs.append(U.random_tx(rng, k, m))
    txs.insert(3, ([], bytes(32), []))
    b = U.Batch(txs)
    return b, U.oracle_batch(b)


@pytest.fixture(scope="module")
def layout_fn():
    return _lib.load().cg_ftx_build_layout


def test_layout_counts_every_small_shape(layout_fn, exhaustive, big):
    for b, exp in (exhaustive, big):
        st, fs, ns = U.layout(layout_fn, b.n_tx, b.comp_start, b.include)
        assert st == _lib.CG_OK
        assert np.array_equal(fs, exp["fcomp_start"]) and np.array_equal(ns, exp["node_start"])
    b, exp = exhaustive
    for t in (0, 1, 5, 1022):  # single transactions: a node count is len(pmt_postorder(pmt_build(...)))
        one = b.rows([t])
        st, fs, ns = U.layout(layout_fn, 1, one.comp_start, one.include)
        assert st == _lib.CG_OK and ns[1] == len(U.oracle_tx(*b.txs[t])[2]) and fs[1] == sum(b.txs[t][2])


def test_layout_argument_errors(layout_fn, exhaustive):
    b, _ = exhaustive
    n, cs, inc = b.n_tx, b.comp_start, b.include
    fs, ns = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    p = U._p
    assert layout_fn(n, p(cs), p(inc), p(fs), p(ns)) == _lib.CG_OK
    assert layout_fn(n, None, p(inc), p(fs), p(ns)) == _lib.CG_E_INVALID_ARGUMENT
    assert layout_fn(n, p(cs), None, p(fs), p(ns)) == _lib.CG_E_INVALID_ARGUMENT
    assert layout_fn(n, p(cs), p(inc), None, p(ns)) == _lib.CG_E_INVALID_ARGUMENT
    assert layout_fn(n, p(cs), p(inc), p(fs), None) == _lib.CG_E_INVALID_ARGUMENT
    for t in (0, 400, n - 1):  # the salt of transaction t included
        bad = inc.copy()
        bad[cs[t + 1] - 1] = 7
        assert layout_fn(n, p(cs), p(bad), p(fs), p(ns)) == _lib.CG_E_INVALID_ARGUMENT
    down = cs.copy()
    down[500] = down[499] - 1
    assert layout_fn(n, p(down), p(inc), p(fs), p(ns)) == _lib.CG_E_INVALID_ARGUMENT
    assert layout_fn(0, p(cs), p(inc), p(fs), p(ns)) == _lib.CG_OK


def test_build_entry_point_refuses_a_null_context(exhaustive):
    b, _ = exhaustive
    lib = _lib.load()
    out = U.alloc_outputs(b.n_tx, 1, 1)
    p = U._p
    st = lib.cg_ftx_build_batch(None, b.n_tx, p(b.arena), len(b.arena), p(b.comp_off), p(b.comp_len), p(b.comp_start),
                                p(b.salts), p(b.include), 1, 1, p(out["fcomp_start"]), p(out["fcomp_index"]),
                                p(out["nonces"]), p(out["node_start"]), p(out["node_kind"]), p(out["node_hash"]),
                                p(out["roots"]))
    assert st == _lib.CG_E_INVALID_ARGUMENT


def test_host_build_of_the_device_code_matches_the_oracle(exhaustive, big):
    lib = U.host_lib()
    for b, exp in (exhaustive, big):
        st, out = U.host_build(lib, b)
        assert st == 0
        U.assert_same(U.trim(out, b.n_tx), exp)
    # the host build's layout is the library's
    b, exp = exhaustive
    st, fs, ns = U.layout(lib.cgf_layout, b.n_tx, b.comp_start, b.include)
    assert st == 0 and np.array_equal(fs, exp["fcomp_start"]) and np.array_equal(ns, exp["node_start"])
    bad = b.include.copy()
    bad[b.comp_start[3] - 1] = 1
    assert U.layout(lib.cgf_layout, b.n_tx, b.comp_start, bad)[0] == -1


def _san_bin():
    path = os.path.join(NATIVE, "ftxbuild_san.bin")
    if not os.path.exists(path):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I",
                               os.path.join(ROOT, "corda_amd", "csrc"), os.path.join(NATIVE, "ftxbuild_san.cpp"),
                               os.path.join(NATIVE, "cg_ftxbuild_host.cpp"), "-o", path])
    return path


def _san_lines(b):
    for comps, salt, inc in b.txs:
        yield "%s %s %s" % (salt.hex(), "".join(str(x) for x in inc) or "-", ",".join(c.hex() for c in comps) or "-")


def test_stand_alone_program_under_asan_ubsan(exhaustive, big):
    """The layout pass and the host-compiled build under ASan + UBSan, as a program of its own
    (nothing is loaded into Python under a sanitizer): two batches, outputs equal the oracle's."""
    text = "\n".join(list(_san_lines(exhaustive[0])) + [""] + list(_san_lines(big[0]))) + "\n"
    run = subprocess.run([_san_bin()], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "2 batches" in run.stderr
    blocks = run.stdout.split("end\n")
    assert len(blocks) == 3 and blocks[2] == ""
    for block, (b, exp) in zip(blocks, (exhaustive, big)):
        f = dict(line.split(" ", 1) if " " in line else (line, "") for line in block.splitlines())
        for name in U.OUT_NAMES:
            assert bytes.fromhex(f[name].strip()) == exp[name].tobytes(), name


def _native(name, build):
    path = os.path.join(NATIVE, name)
    if not os.path.exists(path):
        subprocess.check_call(build + ["-o", path, *LINK])
    return path


def test_plain_c_caller_without_a_device():
    exe = _native("ftx_build_abi.bin", ["gcc", "-std=c99", "-O1", "-Wall", "-Werror", *INCLUDE,
                                        os.path.join(NATIVE, "ftx_build_abi.c")])
    run = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr


def test_jni_harness_cpu_mode():
    exe = _native("jni_ftxbuild_harness.bin",
                  ["gcc", "-std=c99", "-O1", "-Wall", "-Werror", *INCLUDE, "-I",
                   os.path.join(ROOT, "integration", "jvm", "stub"), os.path.join(NATIVE, "jni_ftxbuild_harness.c"),
                   os.path.join(ROOT, "integration", "jvm", "cordagpu_jni.c")])
    run = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
