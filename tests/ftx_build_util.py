"""Shared by tests/test_ftx_build_host.py and tests/test_gpu_ftx_build.py (not a test
module): the exhaustive small (component count, include mask) set, the batch packing of
cg_ftx_build_batch, its expectation from the oracle's restatement
(oracle/py/merkle_tx.py: get_merkle_tree, pmt_build, pmt_postorder, compute_nonce,
leaf_hash) and ctypes callers of the C ABI and of the host build of the device code."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

import merkle_tx as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
OUT_NAMES = ("fcomp_start", "fcomp_index", "nonces", "node_start", "node_kind", "node_hash", "roots")


class Batch:
    """Transactions in the cg_txid_batch layout plus one include byte per component."""

    def __init__(self, txs):
        """txs: list of (components: list[bytes], salt: bytes, include: list[int])."""
        self.txs = txs
        comps = [c for t in txs for c in t[0]]
        self.n_tx = len(txs)
        self.comp_len = np.array([len(c) for c in comps] or [0], dtype=np.uint32)
        self.comp_off = np.zeros(max(len(comps), 1), dtype=np.uint64)
        if len(comps) > 1:
            self.comp_off[1:len(comps)] = np.cumsum(self.comp_len[:len(comps) - 1], dtype=np.uint64)
        self.comp_start = np.zeros(len(txs) + 1, dtype=np.uint32)
        self.comp_start[1:] = np.cumsum([len(t[0]) for t in txs])
        self.arena = np.frombuffer(b"".join(comps) + b"\0", dtype=np.uint8).copy()
        self.salts = np.frombuffer(b"".join(t[1] for t in txs), dtype=np.uint8).copy()
        self.include = np.array([x for t in txs for x in t[2]] or [0], dtype=np.uint8)
        assert all(len(t[0]) == len(t[2]) for t in txs)

    def rows(self, idx):
        return Batch([self.txs[i] for i in idx])


def random_tx(rng, k, include):
    """k components (the last stands for the serialized salt) of assorted lengths, among them
    the SHA-256 padding boundaries of ser || nonce (23/24 and 87/88 bytes)."""
    lens = rng.choice([1, 7, 23, 24, 40, 44, 55, 56, 64, 87, 88, 119, 200], size=k)
    return [rng.bytes(int(n)) for n in lens], rng.bytes(32), list(include)


def exhaustive_txs(seed=20240607):
    """Every (k, mask): k = 1 .. 10 components, every mask over the k - 1 non-salt ones: 1,023."""
    rng = np.random.default_rng(seed)
    txs = []
    for k in range(1, 11):
        for m in range(1 << (k - 1)):
            txs.append(random_tx(rng, k, [(m >> i) & 1 for i in range(k - 1)] + [0]))
    assert len(txs) == 1023
    return txs


def oracle_tx(comps, salt, include):
    """(filtered indices, their nonces, post-order program, root) of one transaction."""
    if not comps:
        return [], [], [], bytes(32)
    k = len(comps)
    leaves = [M.leaf_hash(c, salt, i, i == k - 1) for i, c in enumerate(comps)]
    vis = [i for i in range(k) if include[i]]
    assert len(set(leaves)) == k  # inclusion by index == inclusion by hash value
    tree = M.get_merkle_tree(leaves)
    prog = M.pmt_postorder(M.pmt_build(tree, [leaves[i] for i in vis]))
    return vis, [M.compute_nonce(salt, i) for i in vis], prog, tree.hash


def oracle_batch(b: Batch) -> dict:
    fs, ns, fi, nonces, kinds, hashes, roots = [0], [0], [], [], [], [], []
    for t, (comps, salt, include) in enumerate(b.txs):
        vis, nn, prog, root = oracle_tx(comps, salt, include)
        fi += [int(b.comp_start[t]) + i for i in vis]
        nonces += nn
        kinds += [k for k, _ in prog]
        hashes += [h for _, h in prog]
        roots.append(root)
        fs.append(len(fi))
        ns.append(len(kinds))
    return dict(fcomp_start=np.array(fs, dtype=np.uint32), fcomp_index=np.array(fi, dtype=np.uint32),
                nonces=np.frombuffer(b"".join(nonces), dtype=np.uint8),
                node_start=np.array(ns, dtype=np.uint32), node_kind=np.array(kinds, dtype=np.uint8),
                node_hash=np.frombuffer(b"".join(hashes), dtype=np.uint8),
                roots=np.frombuffer(b"".join(roots), dtype=np.uint8))


def _p(a):
    return None if a is None else a.ctypes.data


def layout(fn, n_tx, comp_start, include, with_ctx=False):
    """cg_ftx_build_layout (or the host build's cgf_layout): (status, fcomp_start, node_start)."""
    fs = np.full(n_tx + 1, 0xdeadbeef, dtype=np.uint32)
    ns = np.full(n_tx + 1, 0xdeadbeef, dtype=np.uint32)
    st = fn(n_tx, _p(comp_start), _p(include), _p(fs), _p(ns))
    return st, fs, ns


def alloc_outputs(n_tx, n_f, n_n, fill=0xa5):
    return dict(fcomp_start=np.full(n_tx + 1, fill * 0x01010101, dtype=np.uint32),
                fcomp_index=np.full(max(n_f, 1), fill * 0x01010101, dtype=np.uint32),
                nonces=np.full(32 * max(n_f, 1), fill, dtype=np.uint8),
                node_start=np.full(n_tx + 1, fill * 0x01010101, dtype=np.uint32),
                node_kind=np.full(max(n_n, 1), fill, dtype=np.uint8),
                node_hash=np.full(32 * max(n_n, 1), fill, dtype=np.uint8),
                roots=np.full(32 * max(n_tx, 1), fill, dtype=np.uint8))


def trim(out, n_tx):
    """The outputs cut to the lengths their start arrays give."""
    n_f, n_n = int(out["fcomp_start"][n_tx]), int(out["node_start"][n_tx])
    return dict(fcomp_start=out["fcomp_start"], fcomp_index=out["fcomp_index"][:n_f], nonces=out["nonces"][:32 * n_f],
                node_start=out["node_start"], node_kind=out["node_kind"][:n_n], node_hash=out["node_hash"][:32 * n_n],
                roots=out["roots"][:32 * n_tx])


def gpu_build(ctx, b: Batch, n_f=None, n_n=None, out=None, **override):
    """cg_ftx_build_batch on batch b with capacities (n_f, n_n) (default: what
    cg_ftx_build_layout says).  Returns (status, outputs as allocated)."""
    if n_f is None or n_n is None:
        st, fs, ns = layout(ctx.lib.cg_ftx_build_layout, b.n_tx, b.comp_start, b.include)
        assert st == 0
        n_f = int(fs[b.n_tx]) if n_f is None else n_f
        n_n = int(ns[b.n_tx]) if n_n is None else n_n
    out = out or alloc_outputs(b.n_tx, n_f, n_n)
    a = dict(arena=b.arena, arena_bytes=len(b.arena), comp_off=b.comp_off, comp_len=b.comp_len,
             comp_start=b.comp_start, salts=b.salts, include=b.include)
    a.update(override)
    st = ctx.lib.cg_ftx_build_batch(ctx.h, b.n_tx, _p(a["arena"]), a["arena_bytes"], _p(a["comp_off"]),
                                    _p(a["comp_len"]), _p(a["comp_start"]), _p(a["salts"]), _p(a["include"]), n_f, n_n,
                                    _p(out["fcomp_start"]), _p(out["fcomp_index"]), _p(out["nonces"]),
                                    _p(out["node_start"]), _p(out["node_kind"]), _p(out["node_hash"]),
                                    _p(out["roots"]))
    return st, out


def assert_same(got: dict, exp: dict, what=""):
    for name in OUT_NAMES:
        g, e = np.asarray(got[name]), np.asarray(exp[name])
        assert g.shape == e.shape, f"{what}{name}: {g.shape} != {e.shape}"
        if not np.array_equal(g, e):
            bad = np.flatnonzero(g != e)
            raise AssertionError(f"{what}{name} differs at {bad[:8]} ({len(bad)} places)")


def host_lib():
    """The host build of the device code (tests/native/cg_ftxbuild_host.cpp)."""
    path = os.path.join(NATIVE, "libcg_ftxbuild_host.so")
    if not os.path.exists(path):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "corda_amd", "csrc"), os.path.join(NATIVE, "cg_ftxbuild_host.cpp"),
                               "-o", path])
    lib = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.cgf_layout.argtypes = [sz, vp, vp, vp, vp]
    lib.cgf_build.argtypes = [sz] + [vp] * 13
    return lib


def host_build(lib, b: Batch):
    st, fs, ns = layout(lib.cgf_layout, b.n_tx, b.comp_start, b.include)
    assert st == 0
    out = alloc_outputs(b.n_tx, int(fs[b.n_tx]), int(ns[b.n_tx]))
    st = lib.cgf_build(b.n_tx, _p(b.arena), _p(b.comp_off), _p(b.comp_len), _p(b.comp_start), _p(b.salts),
                       _p(b.include), _p(out["fcomp_start"]), _p(out["fcomp_index"]), _p(out["nonces"]),
                       _p(out["node_start"]), _p(out["node_kind"]), _p(out["node_hash"]), _p(out["roots"]))
    return st, out
