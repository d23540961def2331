"""cg_ftx_build_batch on the device: the batch FilteredTransaction builder
(wtx.buildFilteredTransaction: MerkleTransaction.kt:159-166, PartialMerkleTree.kt:66-123)
byte for byte against the oracle's restatement (oracle/py/merkle_tx.py), round trips
through cg_ftx_verify_batch, the error contract, the Python mirror and a plain-C caller."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import ftx_build_util as U
import merkle_tx as M
from corda_amd import _lib
from corda_amd import transactions as T
from corda_amd._lib import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "datagen"))

import datagen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exhaustive():
    b = U.Batch(U.exhaustive_txs())
    return b, U.oracle_batch(b)


def txids(ctx, b):
    ids = np.zeros(32 * b.n_tx, dtype=np.uint8)
    st = ctx.lib.cg_txid_batch(ctx.h, b.n_tx, ptr(b.arena), len(b.arena), ptr(b.comp_off), ptr(b.comp_len),
                               ptr(b.comp_start), ptr(b.salts), ptr(ids))
    assert st in (_lib.CG_OK, _lib.CG_E_MERKLE_EMPTY)
    return ids


def verify_built(ctx, arena, comp_off, comp_len, n_tx, out):
    """The build's outputs handed to cg_ftx_verify_batch: the same arena, offsets and lengths
    gathered with fcomp_index."""
    o = U.trim(out, n_tx)
    idx = o["fcomp_index"]
    off = np.ascontiguousarray(comp_off[idx]) if len(idx) else np.zeros(1, np.uint64)
    ln = np.ascontiguousarray(comp_len[idx]) if len(idx) else np.zeros(1, np.uint32)
    res = np.full(n_tx, 9, dtype=np.uint8)
    ctx.check(ctx.lib.cg_ftx_verify_batch(ctx.h, n_tx, ptr(arena), len(arena), ptr(off), ptr(ln),
                                          ptr(o["fcomp_start"]), ptr(out["nonces"]), ptr(o["node_start"]),
                                          ptr(out["node_kind"]), ptr(out["node_hash"]), ptr(out["roots"]), ptr(res)))
    return res


def test_exhaustive_small_shapes(gpu_ctx, exhaustive):
    """Every (k, mask), k = 1 .. 10, in one batch: all outputs byte-identical to the oracle's,
    roots equal to cg_txid_batch's ids; then a sample of rows alone (no cross-row state)."""
    b, exp = exhaustive
    st, out = U.gpu_build(gpu_ctx, b)
    assert st == _lib.CG_OK, gpu_ctx.lib.cg_last_error(gpu_ctx.h)
    U.assert_same(U.trim(out, b.n_tx), exp)
    assert np.array_equal(out["roots"], txids(gpu_ctx, b))
    res = verify_built(gpu_ctx, b.arena, b.comp_off, b.comp_len, b.n_tx, out)
    empty = np.diff(exp["fcomp_start"]) == 0
    assert (res[empty] == _lib.FTX_NO_LEAVES).all() and (res[~empty] == _lib.FTX_TRUE).all()
    for t in (0, 1, 2, 3, 6, 100, 511, 512, 777, 1022):
        one = b.rows([t])
        st, o1 = U.gpu_build(gpu_ctx, one)
        assert st == _lib.CG_OK
        U.assert_same(U.trim(o1, 1), U.oracle_batch(one), f"row {t} alone: ")


def _mask(k, idx):
    m = [0] * k
    for i in idx:
        m[i] = 1
    return m


EDGE = {
    "salt_only": [(1, [])],
    "k2": [(2, []), (2, [0])],
    "pow2_m3": [(8, [0]), (8, [6]), (9, [7]), (9, [0, 7]), (9, [])],
    "pow2_m8": [(256, [0, 254]), (257, [255]), (257, [3, 128])],
    "empty_masks": [(5, []), (16, []), (17, [])],
    "all_included": [(2, [0]), (7, range(6)), (8, range(7)), (33, range(32))],
    "k300_host_check": [(300, range(0, 299)), (300, range(20, 290))],
    "k1000_sparse": [(1000, [0, 517, 998])],
}


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_shapes(gpu_ctx, name):
    rng = np.random.default_rng(sum(name.encode()))
    b = U.Batch([U.random_tx(rng, k, _mask(k, idx)) for k, idx in EDGE[name]])
    exp = U.oracle_batch(b)
    st, out = U.gpu_build(gpu_ctx, b)
    assert st == _lib.CG_OK, gpu_ctx.lib.cg_last_error(gpu_ctx.h)
    U.assert_same(U.trim(out, b.n_tx), exp)
    assert np.array_equal(out["roots"], txids(gpu_ctx, b))
    if name == "salt_only":  # the single node Leaf(root)
        assert exp["node_kind"].tolist() == [1] and np.array_equal(exp["node_hash"], exp["roots"])
    if name == "k300_host_check":  # more included leaves than the verifier checks in one lane
        assert (np.diff(exp["fcomp_start"]) > 256).all()
    res = verify_built(gpu_ctx, b.arena, b.comp_off, b.comp_len, b.n_tx, out)
    want = np.where(np.diff(exp["fcomp_start"]) == 0, _lib.FTX_NO_LEAVES, _lib.FTX_TRUE)
    assert np.array_equal(res, want)


@pytest.fixture(scope="module")
def config4():
    """3,000 config-4 transactions, their leaf hashes from the oracle's functions (once)."""
    w = datagen.make_tx_batch(3000, seed=17, tamper_frac=0.0)
    leaves = []
    for t in range(w.n_tx):
        c0, c1 = int(w.comp_start[t]), int(w.comp_start[t + 1])
        salt = w.salts[32 * t:32 * t + 32].tobytes()
        leaves.append([M.leaf_hash(w.arena[int(w.comp_off[c]):int(w.comp_off[c]) + int(w.comp_len[c])].tobytes(), salt,
                                   c - c0, c == c1 - 1) for c in range(c0, c1)])
    return w, leaves


@pytest.fixture(params=[None, 600], ids=["one_chunk", "five_chunks"])
def build_chunks(request, knobs):
    """The tree pass in one chunk, and forced into 5 chunks of 600 transactions."""
    if request.param:
        knobs.setenv("CORDA_AMD_FTX_BUILD_CHUNK", request.param)
    return request.param


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_round_trip_config4(gpu_ctx, config4, build_chunks, density):
    """Random masks over config-4 transactions: programs and roots equal
    datagen._partial_postorder over the oracle's leaf hashes, and cg_ftx_verify_batch accepts
    every built transaction (NO_LEAVES for an empty mask)."""
    w, leaves = config4
    rng = np.random.default_rng(int(density * 100))
    include = (rng.random(len(w.comp_len)) < density).astype(np.uint8)
    include[w.comp_start[1:] - 1] = 0  # never the salt
    include[w.comp_start[5]:w.comp_start[6]] = 0  # and one certainly empty mask
    n = w.n_tx
    st, fs, ns = U.layout(gpu_ctx.lib.cg_ftx_build_layout, n, w.comp_start, include)
    assert st == 0
    out = U.alloc_outputs(n, int(fs[n]), int(ns[n]))
    st = gpu_ctx.lib.cg_ftx_build_batch(gpu_ctx.h, n, ptr(w.arena), len(w.arena), ptr(w.comp_off), ptr(w.comp_len),
                                        ptr(w.comp_start), ptr(w.salts), ptr(include), int(fs[n]), int(ns[n]),
                                        ptr(out["fcomp_start"]), ptr(out["fcomp_index"]), ptr(out["nonces"]),
                                        ptr(out["node_start"]), ptr(out["node_kind"]), ptr(out["node_hash"]),
                                        ptr(out["roots"]))
    assert st == _lib.CG_OK, gpu_ctx.lib.cg_last_error(gpu_ctx.h)
    kinds, hashes, roots, nst = [], [], [], [0]
    for t in range(n):
        c0 = int(w.comp_start[t])
        inc = {h for i, h in enumerate(leaves[t]) if include[c0 + i]}
        root, prog = datagen._partial_postorder(leaves[t], inc)
        kinds += [k for k, _ in prog]
        hashes += [h for _, h in prog]
        roots.append(root)
        nst.append(len(kinds))
    o = U.trim(out, n)
    assert np.array_equal(o["node_start"], np.array(nst, dtype=np.uint32))
    assert np.array_equal(o["node_kind"], np.array(kinds, dtype=np.uint8))
    assert o["node_hash"].tobytes() == b"".join(hashes)
    assert o["roots"].tobytes() == b"".join(roots) == w.ids.tobytes()
    assert np.array_equal(o["fcomp_index"], np.flatnonzero(include).astype(np.uint32))
    res = verify_built(gpu_ctx, w.arena, w.comp_off, w.comp_len, n, out)
    empty = np.diff(o["fcomp_start"]) == 0
    assert empty[5] and (res[empty] == _lib.FTX_NO_LEAVES).all() and (res[~empty] == _lib.FTX_TRUE).all()


def test_errors_leave_the_context_usable(gpu_ctx, exhaustive):
    b, exp = exhaustive
    b = b.rows(range(200, 260))
    exp = U.oracle_batch(b)
    n_f, n_n = int(exp["fcomp_start"][-1]), int(exp["node_start"][-1])

    def err():
        return (gpu_ctx.lib.cg_last_error(gpu_ctx.h) or b"").decode()

    def good():
        st, out = U.gpu_build(gpu_ctx, b)
        assert st == _lib.CG_OK, err()
        U.assert_same(U.trim(out, b.n_tx), exp)

    def untouched(out):
        return all((a.view(np.uint8) == 0xa5).all() for a in out.values() if a is not None)  # alloc_outputs' fill

    # the salt of transaction 7 included
    inc = b.include.copy()
    inc[b.comp_start[8] - 1] = 1
    st, out = U.gpu_build(gpu_ctx, b, n_f + 1, n_n + 8, include=inc)
    assert st == _lib.CG_E_INVALID_ARGUMENT and "transaction 7" in err() and untouched(out)
    good()
    # capacities one short: nothing written, the message carries the needed counts
    for cf, cn in ((n_f - 1, n_n), (n_f, n_n - 1)):
        st, out = U.gpu_build(gpu_ctx, b, cf, cn)
        assert st == _lib.CG_E_INVALID_ARGUMENT and untouched(out)
        assert str(n_f) in err() and str(n_n) in err()
        good()
    # decreasing comp_start
    cs = b.comp_start.copy()
    cs[10] = cs[9] - 1
    st, out = U.gpu_build(gpu_ctx, b, n_f, n_n, comp_start=cs)
    assert st == _lib.CG_E_INVALID_ARGUMENT and "monotone" in err() and untouched(out)
    good()
    # a component past the arena (also one whose offset + length wraps)
    for c, off in ((17, len(b.arena) - 1), (3, 2**64 - 4)):
        co = b.comp_off.copy()
        co[c] = off
        st, out = U.gpu_build(gpu_ctx, b, n_f, n_n, comp_off=co)
        assert st == _lib.CG_E_INVALID_ARGUMENT and f"component {c}" in err() and untouched(out)
        good()
    # null pointers
    for name in ("comp_start", "salts", "include", "comp_off", "comp_len", "arena"):
        st, out = U.gpu_build(gpu_ctx, b, n_f, n_n, **{name: None})
        assert st == _lib.CG_E_INVALID_ARGUMENT and untouched(out), name
    for name in U.OUT_NAMES:
        o = U.alloc_outputs(b.n_tx, n_f, n_n)
        keep = o[name]
        o[name] = None
        st, _ = U.gpu_build(gpu_ctx, b, n_f, n_n, out=o)
        o[name] = keep
        assert st == _lib.CG_E_INVALID_ARGUMENT and untouched(o), name
    good()


def test_empty_transaction_is_merkle_empty_with_the_rest_written(gpu_ctx, exhaustive):
    b, _ = exhaustive
    txs = [b.txs[i] for i in (300, 301)] + [([], bytes(32), [])] + [b.txs[i] for i in (700, 5)]
    e = U.Batch(txs)
    exp = U.oracle_batch(e)
    assert exp["node_start"][3] == exp["node_start"][2] and not exp["roots"][64:96].any()
    st, out = U.gpu_build(gpu_ctx, e)
    assert st == _lib.CG_E_MERKLE_EMPTY
    U.assert_same(U.trim(out, e.n_tx), exp)


def test_injected_allocation_failures(gpu_ctx, exhaustive):
    b, _ = exhaustive
    b = b.rows(range(500, 540))
    exp = U.oracle_batch(b)
    seen_ok = False
    for k in range(1, 24):
        gpu_ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, k)
        st, _ = U.gpu_build(gpu_ctx, b)
        gpu_ctx.set_debug(_lib.DEBUG_FAIL_ALLOC, 0)
        if st == _lib.CG_OK:  # fewer than k allocations in the call
            seen_ok = True
            break
        assert st == _lib.CG_E_OUT_OF_MEMORY, k
        st, out = U.gpu_build(gpu_ctx, b)
        assert st == _lib.CG_OK
        U.assert_same(U.trim(out, b.n_tx), exp, f"after failed allocation {k}: ")
    assert seen_ok and k > 10


def test_python_mirror(gpu_ctx, exhaustive):
    b, _ = exhaustive
    pick = [1, 2, 9, 40, 41, 300, 640, 1000, 1022]
    wtxs = [T.WireTx(list(b.txs[i][0]), b.txs[i][1]) for i in pick]
    masks = [b.txs[i][2] for i in pick]
    ftxs = T.build_filtered_batch(gpu_ctx, wtxs, masks)
    ids = T.tx_ids(gpu_ctx, wtxs)
    for w, m, f, txid in zip(wtxs, masks, ftxs, ids):
        k = len(w.components)
        leaves = [M.leaf_hash(c, w.salt, i, i == k - 1) for i, c in enumerate(w.components)]
        vis = [i for i in range(k) if m[i]]
        want = T.PartialMerkleTree.build(M.get_merkle_tree(leaves), [leaves[i] for i in vis])
        assert f.partial_merkle_tree.root == want.root  # dataclass equality: the whole tree
        assert f.root_hash == txid
        assert f.filtered_leaves.components == [w.components[i] for i in vis]
        assert f.filtered_leaves.nonces == [M.compute_nonce(w.salt, i) for i in vis]
        if vis:
            assert f.verify(gpu_ctx) is True
        else:
            assert f.partial_merkle_tree.root == T.Leaf(txid)
            with pytest.raises(T.MerkleTreeException):
                f.verify(gpu_ctx)
    one = wtxs[5].build_filtered_transaction(gpu_ctx, masks[5])
    assert (one.root_hash, one.filtered_leaves, one.partial_merkle_tree.root) == (
        ftxs[5].root_hash, ftxs[5].filtered_leaves, ftxs[5].partial_merkle_tree.root)
    assert one.verify(gpu_ctx) is True
    with pytest.raises(T.IllegalArgumentException):
        wtxs[5].build_filtered_transaction(gpu_ctx, masks[5][:-1] + [1])
    with pytest.raises(T.IllegalArgumentException):
        wtxs[5].build_filtered_transaction(gpu_ctx, masks[5][:-1])
    with pytest.raises(T.MerkleTreeException):
        T.build_filtered_batch(gpu_ctx, [wtxs[0], T.WireTx([], bytes(32))], [masks[0], []])


def test_plain_c_caller(gpu_ctx):
    """tests/native/ftx_build_abi.c: one cg_ftx_build_layout + cg_ftx_build_batch call from
    C99 through include/cordagpu.h; it prints its inputs and outputs, checked here against
    the oracle."""
    exe = os.path.join(ROOT, "tests", "native", "ftx_build_abi.bin")
    assert os.path.exists(exe), "ftx_build_abi.bin not built (__graft_entry__.build())"
    run = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    f = dict(line.split(" ", 1) for line in run.stdout.splitlines() if " " in line)
    counts = [int(x) for x in f["counts"].split()]
    lens = [int(x) for x in f["comp_len"].split()]
    arena, salts, include = bytes.fromhex(f["arena"]), bytes.fromhex(f["salts"]), bytes.fromhex(f["include"])
    txs, c, off = [], 0, 0
    for t, k in enumerate(counts):
        comps = []
        for n in lens[c:c + k]:
            comps.append(arena[off:off + n])
            off += n
        txs.append((comps, salts[32 * t:32 * t + 32], list(include[c:c + k])))
        c += k
    exp = U.oracle_batch(U.Batch(txs))
    assert [int(x) for x in f["fcomp_start"].split()] == exp["fcomp_start"].tolist()
    assert [int(x) for x in f["fcomp_index"].split()] == exp["fcomp_index"].tolist()
    assert [int(x) for x in f["node_start"].split()] == exp["node_start"].tolist()
    assert bytes.fromhex(f["node_kind"]) == exp["node_kind"].tobytes()
    assert bytes.fromhex(f["node_hash"]) == exp["node_hash"].tobytes()
    assert bytes.fromhex(f["nonces"]) == exp["nonces"].tobytes()
    assert bytes.fromhex(f["roots"]) == exp["roots"].tobytes()


def test_jni_glue_builds_on_the_device():
    """integration/jvm/cordagpu_jni.c's nativeFtxBuildLayout / buildFilteredBatch driven by a
    fake JNIEnv (tests/native/jni_ftxbuild_harness.c), with the round trip through nativeFtxVerify."""
    exe = os.path.join(ROOT, "tests", "native", "jni_ftxbuild_harness.bin")
    assert os.path.exists(exe), "jni_ftxbuild_harness.bin not built (__graft_entry__.build())"
    run = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
