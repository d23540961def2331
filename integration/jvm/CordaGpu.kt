// JVM-side binding of libcordagpu for Corda 0.14 (core/src/main/kotlin/net/corda/core/crypto/).
// NOT compiled in this repository's CI: the build image has no JDK/Kotlin toolchain.
// Written against the reference's Kotlin 1.1.1 stdlib (constants.properties:2): no
// maxOfOrNull / sumOf / flatMapIndexed.  The C side it binds is include/cordagpu.h; the
// JNI glue is cordagpu_jni.c (exercised without a JDK by tests/native/jni_harness.c).
package net.corda.core.crypto.gpu

import net.corda.core.contracts.PrivacySalt
import net.corda.core.crypto.Crypto
import net.corda.core.crypto.DigitalSignature
import net.corda.core.crypto.MerkleTreeException
import net.corda.core.crypto.PartialMerkleTree
import net.corda.core.crypto.SignatureScheme
import net.corda.core.crypto.TransactionSignature
import net.corda.core.crypto.composite.CompositeKey
import net.corda.core.serialization.SerializationDefaults.P2P_CONTEXT
import net.corda.core.serialization.serialize
import net.corda.core.transactions.SignedTransaction
import net.corda.core.transactions.WireTransaction
import java.nio.ByteBuffer
import java.nio.ByteOrder
import java.security.InvalidKeyException
import java.math.BigInteger
import java.security.PublicKey
import java.security.SecureRandom
import java.security.SignatureException
import java.security.interfaces.ECPrivateKey
import java.security.interfaces.ECPublicKey
import net.corda.core.crypto.SecureHash
import net.i2p.crypto.eddsa.EdDSAPrivateKey
import net.i2p.crypto.eddsa.EdDSAPublicKey

/** Verdict codes of cg_verify_batch (include/cordagpu.h). */
object Verdict {
    const val ACCEPT = 0; const val REJECT = 1; const val SIG_MALFORMED = 2
    const val KEY_INVALID = 3; const val ARG_EMPTY = 4; const val UNSUPPORTED = 5
}

/** Per-tx codes of cg_tx_verify_batch / cg_tx_verify_signatures_except (>= 0: first bad signature). */
object TxStatus {
    const val OK = -1; const val NO_SIGNATURES = -2; const val NO_COMPONENTS = -3; const val SIGNATURES_MISSING = -4
}

/** Schemes the device runs (SignatureScheme.schemeNumberID, Crypto.kt:92,106,120). */
val GPU_SCHEMES = setOf(2, 3, 4)

private fun direct(bytes: Int): ByteBuffer = ByteBuffer.allocateDirect(maxOf(bytes, 1)).order(ByteOrder.LITTLE_ENDIAN)

/** One libcordagpu context per thread (a cg_ctx is single-threaded); device = LOCAL_RANK of this JVM. */
class CordaGpu(device: Int = 0) : AutoCloseable {
    private val handle: Long = nativeOpen(device).also { require(it > 0L) { "libcordagpu: no gfx950 device ($it)" } }

    override fun close() = nativeClose(handle)

    private fun check(rc: Int) = check(rc == 0) { "libcordagpu error $rc: ${nativeLastError(handle)}" }

    /** A CORDA_AMD_* tuning knob of this context (cg_set_option; null: the library default). The
     *  library reads the environment only when the context opens; no knob changes a verdict. */
    fun setOption(key: String, value: String?) = check(nativeSetOption(handle, key, value))

    /**
     * Batch form of [Crypto.isValid] (Crypto.kt:534-541) / [Crypto.doVerify] (Crypto.kt:472-483):
     * one verdict byte per element.  Buffers are direct ByteBuffers in the C-ABI layout (see [pack]).
     */
    fun verify(batch: PackedBatch, doVerifyMode: Boolean): ByteArray {
        val out = direct(batch.n)
        check(nativeVerify(handle, batch.n, if (doVerifyMode) 1 else 0, batch.scheme, batch.pk, PK_STRIDE,
                batch.sig, batch.sigStride, batch.sigLen, batch.msg, batch.msgOff, batch.msgLen, out, null))
        return ByteArray(batch.n).also { out.get(it) }
    }

    /** A batch staged once in HBM (a notary backlog): cg_batch_create / cg_batch_verify / cg_batch_destroy. */
    inner class Prepared(batch: PackedBatch) : AutoCloseable {
        private val b: Long = nativeBatchCreate(handle, batch.n, batch.scheme, batch.pk, PK_STRIDE, batch.sig,
                batch.sigStride, batch.sigLen, batch.msg, batch.msgOff, batch.msgLen)
                .also { check(it > 0L) { "libcordagpu error $it: ${nativeLastError(handle)}" } }
        val n = batch.n
        fun verify(doVerifyMode: Boolean): ByteArray {
            val out = direct(n)
            check(nativeBatchVerify(handle, b, if (doVerifyMode) 1 else 0, out, null))
            return ByteArray(n).also { out.get(it) }
        }
        override fun close() = nativeBatchDestroy(handle, b)
    }

    /** Transactions in the cg_tx_verify_batch layout (built by [TxArena.of]). */
    fun txVerify(a: TxArena, sigs: PackedBatch, doVerifyMode: Boolean): IntArray {
        val firstBad = direct(4 * a.nTx)
        val rc = nativeTxVerify(handle, if (doVerifyMode) 1 else 0, a.nTx, a.arena, a.compOff, a.compLen, a.compStart,
                a.salts, a.sigStart, sigs.scheme, sigs.pk, PK_STRIDE, sigs.sig, sigs.sigStride, sigs.sigLen, firstBad,
                null, null)
        check(rc == 0 || rc == CG_E_MERKLE_EMPTY) { "libcordagpu error $rc: ${nativeLastError(handle)}" }
        return IntArray(a.nTx) { firstBad.getInt(4 * it) }
    }

    /**
     * [SignedTransaction.verifySignaturesExcept] for many transactions in one device call
     * (TransactionWithSignatures.kt:41-47, 72-77).  Returns the per-tx [TxStatus] codes and, per tx,
     * the required keys in the SignaturesMissingException set.
     */
    fun txVerifySignaturesExcept(a: TxArena, sigs: PackedBatch, req: RequiredKeys): Pair<IntArray, List<List<PublicKey>>> {
        val status = direct(4 * a.nTx)
        val missing = direct(req.keys.size)
        val rc = nativeTxVerifyExcept(handle, 1, a.nTx, a.arena, a.compOff, a.compLen, a.compStart, a.salts, a.sigStart,
                sigs.scheme, sigs.pk, PK_STRIDE, sigs.sig, sigs.sigStride, sigs.sigLen, req.reqStart, req.progStart,
                req.prog, req.allowed, status, missing, null)
        check(rc == 0 || rc == CG_E_MERKLE_EMPTY) { "libcordagpu error $rc: ${nativeLastError(handle)}" }
        val codes = IntArray(a.nTx) { status.getInt(4 * it) }
        val miss = (0 until a.nTx).map { t ->
            (req.reqStart.getInt(4 * t) until req.reqStart.getInt(4 * t + 4)).filter { missing.get(it).toInt() != 0 }
                    .map { req.keys[it] }
        }
        return Pair(codes, miss)
    }

    /**
     * A loop of `wtx.buildFilteredTransaction(filtering)` (WireTransaction.kt:97-98 ->
     * FilteredTransaction.buildMerkleTransaction, MerkleTransaction.kt:159-166 -> PartialMerkleTree.build,
     * PartialMerkleTree.kt:66-123) in one device call: cg_ftx_build_layout sizes the outputs on the host,
     * cg_ftx_build_batch fills them.  include: one byte per component of the arena, non-zero where the
     * filtering predicate accepted it (never on a transaction's last component, the privacy salt:
     * IllegalArgumentException).  A transaction without components: MerkleTreeException, as
     * MerkleTree.getMerkleTree throws.
     */
    fun buildFilteredBatch(a: TxArena, include: ByteBuffer): FilteredBatch {
        val fStart = direct(4 * (a.nTx + 1)); val nStart = direct(4 * (a.nTx + 1))
        require(nativeFtxBuildLayout(a.nTx, a.compStart, include, fStart, nStart) == 0) {
            "the include mask selects a privacy salt, or the component ranges are not monotone"
        }
        val nF = fStart.getInt(4 * a.nTx); val nN = nStart.getInt(4 * a.nTx)
        val out = FilteredBatch(a.nTx, fStart, direct(4 * nF), direct(32 * nF), nStart, direct(nN), direct(32 * nN),
                direct(32 * a.nTx))
        val rc = buildFilteredBatch(handle, a.nTx, a.arena, a.compOff, a.compLen, a.compStart, a.salts, include,
                out.fcompStart, out.fcompIndex, out.nonces, out.nodeStart, out.nodeKind, out.nodeHash, out.roots)
        if (rc == CG_E_MERKLE_EMPTY) throw MerkleTreeException("Cannot calculate Merkle root on empty hash list.")
        check(rc)
        return out
    }

    /**
     * cg_ftx_build_batch's outputs: per tx its filtered components (batch-global component indices and
     * their nonces), its partial tree as the post-order program cg_ftx_verify_batch takes, and its root.
     */
    class FilteredBatch(val nTx: Int, val fcompStart: ByteBuffer, val fcompIndex: ByteBuffer, val nonces: ByteBuffer,
                        val nodeStart: ByteBuffer, val nodeKind: ByteBuffer, val nodeHash: ByteBuffer,
                        val roots: ByteBuffer) {
        private fun hash(b: ByteBuffer, j: Int) = SecureHash.SHA256(ByteArray(32).also { b.position(32 * j); b.get(it) })

        fun rootHash(t: Int): SecureHash = hash(roots, t)
        /** Indices, within tx t's availableComponents, of its filtered components (compStart: the arena's). */
        fun visible(t: Int, compStart: ByteBuffer): List<Int> =
                (fcompStart.getInt(4 * t) until fcompStart.getInt(4 * t + 4)).map { fcompIndex.getInt(4 * it) - compStart.getInt(4 * t) }
        fun nonces(t: Int): List<SecureHash> = (fcompStart.getInt(4 * t) until fcompStart.getInt(4 * t + 4)).map { hash(nonces, it) }
        /** The PartialMerkleTree of tx t, rebuilt from its post-order program. */
        fun partialMerkleTree(t: Int): PartialMerkleTree {
            val st = ArrayList<PartialMerkleTree.PartialTree>()
            for (j in nodeStart.getInt(4 * t) until nodeStart.getInt(4 * t + 4)) when (nodeKind.get(j).toInt()) {
                0 -> st.add(PartialMerkleTree.PartialTree.IncludedLeaf(hash(nodeHash, j)))
                1 -> st.add(PartialMerkleTree.PartialTree.Leaf(hash(nodeHash, j)))
                else -> { val r = st.removeAt(st.size - 1); val l = st.removeAt(st.size - 1); st.add(PartialMerkleTree.PartialTree.Node(l, r)) }
            }
            return PartialMerkleTree(st.single())
        }
    }

    /**
     * Ed25519 private keys expanded once on the device (cg_signer_create).  A key goes over as its
     * 32-byte seed, the form Ed25519PrivateKeySerializer writes (Kryo.kt:316-320); the direct buffer
     * that carried the seeds is zeroed before the constructor returns.
     */
    inner class Signer(privateKeys: List<EdDSAPrivateKey>) : AutoCloseable {
        val n = privateKeys.size
        private val s: Long
        init {
            val seeds = direct(32 * n)
            privateKeys.forEach { seeds.put(it.seed) }
            try {
                s = nativeSignerCreate(handle, n, seeds)
            } finally {
                for (i in 0 until 32 * n) seeds.put(i, 0)
            }
            check(s > 0L) { "libcordagpu error $s: ${nativeLastError(handle)}" }
        }

        /** A (EdDSAPublicKey.abyte) of every key, as the device derived it. */
        fun publicKeys(): List<ByteArray> {
            val out = direct(32 * n)
            check(nativeSignerPublicKeys(handle, s, out))
            return (0 until n).map { j -> ByteArray(32).also { out.position(32 * j); out.get(it) } }
        }

        /**
         * A loop of [Crypto.doSign] (Crypto.kt:394-401) in one device call: clearData[i] signed with key
         * keyIndex[i] (null: key 0).  Throws what the loop would throw first: IllegalArgumentException
         * for the lowest empty element (Crypto.kt:397).
         */
        fun sign(clearData: List<ByteArray>, keyIndex: IntArray? = null): List<ByteArray> {
            val m = clearData.size
            val msg = direct(clearData.sumBy { it.size }); val msgOff = direct(8 * m); val msgLen = direct(4 * m)
            val idx = keyIndex?.let { k -> direct(4 * m).also { b -> k.forEachIndexed { i, v -> b.putInt(4 * i, v) } } }
            var off = 0L
            for (i in 0 until m) {
                msgOff.putLong(8 * i, off); msgLen.putInt(4 * i, clearData[i].size)
                msg.position(off.toInt()); msg.put(clearData[i]); off += clearData[i].size
            }
            val sig = direct(64 * m); val status = direct(m)
            check(signBatch(handle, s, m, idx, msg, msgOff, msgLen, sig, status))
            for (i in 0 until m)
                require(status.get(i).toInt() == SIGN_OK) { "Signing of an empty array is not permitted!" }
            return (0 until m).map { i -> ByteArray(64).also { sig.position(64 * i); sig.get(it) } }
        }

        override fun close() = nativeSignerDestroy(handle, s)
    }

    /**
     * EC private keys of one curve held on the device (cg_ecdsa_signer_create).  scheme: 2
     * (ECDSA_SECP256K1_SHA256) or 3 (ECDSA_SECP256R1_SHA256).  A key goes over as the 32 big-endian bytes of
     * ECPrivateKey.s; the direct buffer that carried them is zeroed before the constructor returns.
     */
    inner class EcdsaSigner(val scheme: Int, privateKeys: List<ECPrivateKey>) : AutoCloseable {
        val n = privateKeys.size
        private val order: BigInteger = privateKeys.firstOrNull()?.params?.order ?: BigInteger.ONE
        private val s: Long
        init {
            val d = direct(32 * n)
            privateKeys.forEach { d.put(be32(it.s)) }
            try {
                s = nativeEcdsaSignerCreate(handle, scheme, n, d)
            } finally {
                for (i in 0 until 32 * n) d.put(i, 0)
            }
            check(s > 0L) { "libcordagpu error $s: ${nativeLastError(handle)}" }
        }

        /** Q = d G of every key as 64 bytes X || Y, the key form nativeVerify takes. */
        fun publicKeys(): List<ByteArray> {
            val out = direct(64 * n)
            check(nativeEcdsaSignerPublicKeys(handle, s, out))
            return (0 until n).map { j -> ByteArray(64).also { out.position(64 * j); out.get(it) } }
        }

        /**
         * A loop of [Crypto.doSign] for EC keys in one device call.  BC 1.57's ECDSASigner.generateSignature is a
         * pure function of (d, e, k): with secureRandom given, the nonces are drawn here exactly as
         * RandomDSAKCalculator.nextK draws them — BigInteger(256, secureRandom) until it lies in [1, n-1] — so the
         * DER bytes are the ones BC would have produced from those draws; an element whose nonce gives r = 0 or
         * s = 0 is drawn and signed again, as generateSignature's loop does.  secureRandom = null: RFC 6979 nonces
         * derived on the device (deterministic).  Throws IllegalArgumentException for the lowest empty element
         * (Crypto.kt:397).
         */
        fun sign(clearData: List<ByteArray>, keyIndex: IntArray? = null, secureRandom: SecureRandom? = null): List<ByteArray> {
            val m = clearData.size
            val msg = direct(clearData.sumBy { it.size }); val msgOff = direct(8 * m); val msgLen = direct(4 * m)
            val idx = keyIndex?.let { k -> direct(4 * m).also { b -> k.forEachIndexed { i, v -> b.putInt(4 * i, v) } } }
            var off = 0L
            for (i in 0 until m) {
                msgOff.putLong(8 * i, off); msgLen.putInt(4 * i, clearData[i].size)
                msg.position(off.toInt()); msg.put(clearData[i]); off += clearData[i].size
            }
            val kBe = secureRandom?.let { rnd -> direct(32 * m).also { b -> for (i in 0 until m) b.put(be32(nextK(rnd))) } }
            val sig = direct(ECDSA_SIG_MAX * m); val sigLen = direct(4 * m); val status = direct(m)
            val mode = if (secureRandom == null) ECDSA_NONCE_RFC6979 else ECDSA_NONCE_CALLER
            try {
                check(ecdsaSignBatch(handle, s, m, idx, msg, msgOff, msgLen, mode, kBe, sig, ECDSA_SIG_MAX, sigLen, status))
            } finally {
                kBe?.let { b -> for (i in 0 until 32 * m) b.put(i, 0) }
            }
            val out = arrayOfNulls<ByteArray>(m)
            for (i in 0 until m) {
                val st = status.get(i).toInt()
                require(st != SIGN_EMPTY) { "Signing of an empty array is not permitted!" }
                if (st == SIGN_OK) out[i] = ByteArray(sigLen.getInt(4 * i)).also { sig.position(ECDSA_SIG_MAX * i); sig.get(it) }
            }
            // r = 0 or s = 0 (probability ~2^-255 per draw): generateSignature draws k again
            val again = (0 until m).filter { out[it] == null }
            if (again.isNotEmpty()) {
                check(secureRandom != null) { "degenerate RFC 6979 signature: the key was chosen against the message" }
                val redo = sign(again.map { clearData[it] }, keyIndex?.let { k -> IntArray(again.size) { j -> k[again[j]] } }, secureRandom)
                again.forEachIndexed { j, i -> out[i] = redo[j] }
            }
            return out.map { it!! }
        }

        /** RandomDSAKCalculator.nextK: BigInteger(qBitLength, random) until 1 <= k < n. */
        private fun nextK(rnd: SecureRandom): BigInteger {
            while (true) {
                val k = BigInteger(256, rnd)
                if (k.signum() > 0 && k < order) return k
            }
        }

        override fun close() = nativeEcdsaSignerDestroy(handle, s)
    }

    /** Batch form of [Crypto.doSign]: element i signed with privateKeys[i] (Ed25519 keys only). */
    fun doSignBatch(privateKeys: List<EdDSAPrivateKey>, clearData: List<ByteArray>): List<ByteArray> {
        require(privateKeys.size == clearData.size) { "privateKeys and clearData differ in length" }
        val distinct = privateKeys.distinct()
        val slot = distinct.withIndex().associate { (j, k) -> k to j }
        return Signer(distinct).use { it.sign(clearData, IntArray(clearData.size) { i -> slot[privateKeys[i]]!! }) }
    }

    class PackedBatch(val n: Int, val scheme: ByteBuffer, val pk: ByteBuffer, val sig: ByteBuffer, val sigStride: Int,
                      val sigLen: ByteBuffer, val msg: ByteBuffer, val msgOff: ByteBuffer, val msgLen: ByteBuffer)

    companion object {
        const val PK_STRIDE = 64
        const val CG_E_MERKLE_EMPTY = -5
        const val SIGN_OK = 0; const val SIGN_EMPTY = 1  // cg_sign_batch status bytes
        const val SIGN_NONCE_INVALID = 2; const val SIGN_DEGENERATE = 3  // cg_ecdsa_sign_batch: further status bytes
        const val ECDSA_NONCE_RFC6979 = 0; const val ECDSA_NONCE_CALLER = 1
        const val ECDSA_SIG_MAX = 72  // CG_ECDSA_SIG_MAX: the longest DER signature, the least sig_stride

        /** v as exactly 32 big-endian bytes (0 <= v < 2^256). */
        fun be32(v: BigInteger): ByteArray {
            val raw = v.toByteArray()  // minimal two's complement: at most one leading zero byte above 32
            val out = ByteArray(32)
            val take = minOf(raw.size, 32)
            System.arraycopy(raw, raw.size - take, out, 32 - take, take)
            return out
        }
        init { System.loadLibrary("cordagpu_jni") }

        @JvmStatic external fun nativeOpen(device: Int): Long
        @JvmStatic external fun nativeClose(handle: Long)
        @JvmStatic external fun nativeLastError(handle: Long): String
        @JvmStatic external fun nativeSetOption(handle: Long, key: String, value: String?): Int
        @JvmStatic external fun nativeVerify(handle: Long, n: Int, mode: Int, scheme: ByteBuffer, pk: ByteBuffer,
                                             pkStride: Int, sig: ByteBuffer, sigStride: Int, sigLen: ByteBuffer,
                                             msg: ByteBuffer, msgOff: ByteBuffer, msgLen: ByteBuffer,
                                             verdicts: ByteBuffer, bitmap: ByteBuffer?): Int
        @JvmStatic external fun nativeBatchCreate(handle: Long, n: Int, scheme: ByteBuffer, pk: ByteBuffer, pkStride: Int,
                                                  sig: ByteBuffer, sigStride: Int, sigLen: ByteBuffer, msg: ByteBuffer,
                                                  msgOff: ByteBuffer, msgLen: ByteBuffer): Long
        @JvmStatic external fun nativeBatchVerify(handle: Long, batch: Long, mode: Int, verdicts: ByteBuffer?,
                                                  bitmap: ByteBuffer?): Int
        @JvmStatic external fun nativeBatchDestroy(handle: Long, batch: Long)
        @JvmStatic external fun nativeTxVerify(handle: Long, mode: Int, nTx: Int, arena: ByteBuffer, compOff: ByteBuffer,
                                               compLen: ByteBuffer, compStart: ByteBuffer, salts: ByteBuffer,
                                               sigStart: ByteBuffer, scheme: ByteBuffer, pk: ByteBuffer, pkStride: Int,
                                               sig: ByteBuffer, sigStride: Int, sigLen: ByteBuffer, firstBad: ByteBuffer,
                                               verdicts: ByteBuffer?, ids: ByteBuffer?): Int
        @JvmStatic external fun nativeTxVerifyExcept(handle: Long, mode: Int, nTx: Int, arena: ByteBuffer,
                                                     compOff: ByteBuffer, compLen: ByteBuffer, compStart: ByteBuffer,
                                                     salts: ByteBuffer, sigStart: ByteBuffer, scheme: ByteBuffer,
                                                     pk: ByteBuffer, pkStride: Int, sig: ByteBuffer, sigStride: Int,
                                                     sigLen: ByteBuffer, reqStart: ByteBuffer, progStart: ByteBuffer,
                                                     prog: ByteBuffer, allowed: ByteBuffer, status: ByteBuffer,
                                                     missing: ByteBuffer?, ids: ByteBuffer?): Int
        @JvmStatic external fun nativeFtxVerify(handle: Long, nFtx: Int, arena: ByteBuffer, compOff: ByteBuffer,
                                                compLen: ByteBuffer, compStart: ByteBuffer, nonces: ByteBuffer,
                                                nodeStart: ByteBuffer, nodeKind: ByteBuffer, nodeHash: ByteBuffer,
                                                roots: ByteBuffer, result: ByteBuffer): Int
        @JvmStatic external fun nativeFtxBuildLayout(nTx: Int, compStart: ByteBuffer, include: ByteBuffer,
                                                     fcompStart: ByteBuffer, nodeStart: ByteBuffer): Int
        @JvmStatic external fun buildFilteredBatch(handle: Long, nTx: Int, arena: ByteBuffer, compOff: ByteBuffer,
                                                   compLen: ByteBuffer, compStart: ByteBuffer, salts: ByteBuffer,
                                                   include: ByteBuffer, fcompStart: ByteBuffer, fcompIndex: ByteBuffer,
                                                   nonces: ByteBuffer, nodeStart: ByteBuffer, nodeKind: ByteBuffer,
                                                   nodeHash: ByteBuffer, roots: ByteBuffer): Int
        @JvmStatic external fun nativeSignerCreate(handle: Long, nKeys: Int, seeds: ByteBuffer): Long
        @JvmStatic external fun nativeSignerPublicKeys(handle: Long, signer: Long, pkOut: ByteBuffer): Int
        @JvmStatic external fun nativeSignerDestroy(handle: Long, signer: Long)
        @JvmStatic external fun signBatch(handle: Long, signer: Long, n: Int, keyIndex: ByteBuffer?, msg: ByteBuffer,
                                          msgOff: ByteBuffer, msgLen: ByteBuffer, sigOut: ByteBuffer,
                                          status: ByteBuffer?): Int
        @JvmStatic external fun nativeEcdsaSignerCreate(handle: Long, scheme: Int, nKeys: Int, dBe: ByteBuffer): Long
        @JvmStatic external fun nativeEcdsaSignerPublicKeys(handle: Long, signer: Long, xyOut: ByteBuffer): Int
        @JvmStatic external fun nativeEcdsaSignerDestroy(handle: Long, signer: Long)
        @JvmStatic external fun ecdsaSignBatch(handle: Long, signer: Long, n: Int, keyIndex: ByteBuffer?, msg: ByteBuffer,
                                               msgOff: ByteBuffer, msgLen: ByteBuffer, nonceMode: Int, kBe: ByteBuffer?,
                                               sigOut: ByteBuffer, sigStride: Int, sigLenOut: ByteBuffer,
                                               status: ByteBuffer?): Int
        @JvmStatic external fun nativeCompositeEval(handle: Long, nQ: Int, progStart: ByteBuffer, prog: ByteBuffer,
                                                    nSig: Int, sigStart: ByteBuffer, verdicts: ByteBuffer?,
                                                    out: ByteBuffer): Int

        /** Key bytes as the C ABI wants them: Ed25519 A (Kryo.kt:330-340 wire form), ECDSA affine X||Y. */
        fun keyBytes(pk: PublicKey): ByteArray = when (pk) {
            is EdDSAPublicKey -> pk.abyte
            is ECPublicKey -> ByteArray(64).also { out ->
                val x = pk.w.affineX.toByteArray().takeLast(32).toByteArray()
                val y = pk.w.affineY.toByteArray().takeLast(32).toByteArray()
                System.arraycopy(x, 0, out, 32 - x.size, x.size)
                System.arraycopy(y, 0, out, 64 - y.size, y.size)
            }
            else -> throw IllegalArgumentException("not a device scheme key: ${pk.algorithm}")
        }

        /** Packs the GPU-scheme elements only (callers split off [GPU_SCHEMES] first). */
        fun pack(schemes: List<SignatureScheme>, keys: List<PublicKey>, sigs: List<ByteArray>,
                 data: List<ByteArray>): PackedBatch {
            val n = sigs.size
            val sigStride = (((sigs.map { it.size }.max() ?: 64).coerceAtLeast(64) + 3) / 4) * 4
            val scheme = direct(n); val pk = direct(n * PK_STRIDE); val sig = direct(n * sigStride)
            val sigLen = direct(4 * n); val msgOff = direct(8 * n); val msgLen = direct(4 * n)
            val msg = direct(data.sumBy { it.size })
            var off = 0L
            for (i in 0 until n) {
                scheme.put(i, schemes[i].schemeNumberID.toByte())
                val k = keyBytes(keys[i]); pk.position(i * PK_STRIDE); pk.put(k)
                sig.position(i * sigStride); sig.put(sigs[i]); sigLen.putInt(4 * i, sigs[i].size)
                msgOff.putLong(8 * i, off); msgLen.putInt(4 * i, data[i].size)
                msg.position(off.toInt()); msg.put(data[i]); off += data[i].size
            }
            return PackedBatch(n, scheme, pk, sig, sigStride, sigLen, msg, msgOff, msgLen)
        }
    }
}

// ---------------------------------------------------------------- SURVEY 8(f) row 2: the leaf-arena producer
/**
 * The component bytes of many WireTransactions in the cg_txid_batch / cg_tx_verify_batch layout —
 * produced ONCE per tx with exactly the serialization [net.corda.core.transactions.serializedHash]
 * hashes (MerkleTransaction.kt:23-30: `x.serialize(context = P2P_CONTEXT.withoutReferences()).bytes`,
 * components in availableComponents order :74-87, the privacy salt last), so the device recomputes
 * `WireTransaction.id` (WireTransaction.kt:39) without the JVM hashing anything.
 */
class TxArena(val nTx: Int, val arena: ByteBuffer, val compOff: ByteBuffer, val compLen: ByteBuffer,
              val compStart: ByteBuffer, val salts: ByteBuffer, val sigStart: ByteBuffer) {
    companion object {
        fun of(wtxs: List<WireTransaction>, sigCounts: List<Int>): TxArena {
            val ctx = P2P_CONTEXT.withoutReferences()
            val leaves = wtxs.map { w -> w.availableComponents.map { it.serialize(context = ctx).bytes } }
            val nComp = leaves.sumBy { it.size }
            val arena = direct(leaves.sumBy { l -> l.sumBy { it.size } })
            val compOff = direct(8 * nComp); val compLen = direct(4 * nComp)
            val compStart = direct(4 * (wtxs.size + 1)); val salts = direct(32 * wtxs.size)
            val sigStart = direct(4 * (wtxs.size + 1))
            var c = 0; var off = 0L; var s = 0
            for ((t, l) in leaves.withIndex()) {
                compStart.putInt(4 * t, c); sigStart.putInt(4 * t, s)
                for (bytes in l) {
                    compOff.putLong(8 * c, off); compLen.putInt(4 * c, bytes.size)
                    arena.position(off.toInt()); arena.put(bytes); off += bytes.size; c++
                }
                val salt: PrivacySalt = wtxs[t].privacySalt
                salts.position(32 * t); salts.put(salt.bytes)
                s += sigCounts[t]
            }
            compStart.putInt(4 * wtxs.size, c); sigStart.putInt(4 * wtxs.size, s)
            return TxArena(wtxs.size, arena, compOff, compLen, compStart, salts, sigStart)
        }
    }
}

/**
 * requiredSigningKeys of each tx as cg_composite_eval_batch op programs whose leaves index the tx's
 * own signatures (sigKeys = sigs.map { it.by }, TransactionWithSignatures.kt:73), and the
 * allowedToBeMissing marks.
 */
class RequiredKeys(val keys: List<PublicKey>, val reqStart: ByteBuffer, val progStart: ByteBuffer, val prog: ByteBuffer,
                   val allowed: ByteBuffer) {
    companion object {
        fun of(stxs: List<SignedTransaction>, allowedToBeMissing: List<Set<PublicKey>>): RequiredKeys {
            val keys = ArrayList<PublicKey>(); val ops = ArrayList<IntArray>()
            val reqStart = direct(4 * (stxs.size + 1)); val progStarts = ArrayList<Int>(); val allowed = ArrayList<Byte>()
            for ((t, stx) in stxs.withIndex()) {
                reqStart.putInt(4 * t, keys.size)
                val sigIndex = HashMap<PublicKey, Int>()
                for ((i, s) in stx.sigs.withIndex()) if (s.by !in sigIndex) sigIndex[s.by] = i
                for (k in stx.tx.mustSign) {
                    progStarts.add(ops.size)
                    emit(k, 1, sigIndex, ops)
                    keys.add(k)
                    allowed.add(if (k in allowedToBeMissing[t]) 1 else 0)
                }
            }
            reqStart.putInt(4 * stxs.size, keys.size)
            progStarts.add(ops.size)
            val progStart = direct(4 * progStarts.size); val prog = direct(16 * ops.size); val al = direct(allowed.size)
            for ((i, p) in progStarts.withIndex()) progStart.putInt(4 * i, p)
            for ((i, op) in ops.withIndex()) for (j in 0..3) prog.putInt(16 * i + 4 * j, op[j])
            for ((i, a) in allowed.withIndex()) al.put(i, a)
            return RequiredKeys(keys, reqStart, progStart, prog, al)
        }

        /** Post-order {LEAF, sig, weight, 0} / {NODE, arity, weight, threshold} (CompositeKey.kt:186-209). */
        private fun emit(k: PublicKey, weight: Int, sigIndex: Map<PublicKey, Int>, ops: MutableList<IntArray>) {
            if (k is CompositeKey) {
                for (c in k.children) emit(c.node, c.weight, sigIndex, ops)
                ops.add(intArrayOf(1, k.children.size, weight, k.threshold))
            } else {
                ops.add(intArrayOf(0, sigIndex[k] ?: -1, weight, 0))
            }
        }
    }
}

// ---------------------------------------------------------------- Crypto batch surface
// Mirrors Crypto.isValid / Crypto.doVerify one element at a time (Crypto.kt:472-541).

private val gpu = ThreadLocal.withInitial { CordaGpu(System.getenv("LOCAL_RANK")?.toInt() ?: 0) }

/**
 * Verdict codes for every element: GPU schemes (2/3/4) in one device batch, every other scheme
 * Crypto supports (RSA_SHA256, SPHINCS-256, COMPOSITE — Crypto.kt:176-183) through the JVM's own
 * Crypto.isValid / doVerify, merged back in index order.
 */
private fun verdicts(schemes: List<SignatureScheme>, keys: List<PublicKey>, sigs: List<ByteArray>,
                     data: List<ByteArray>, doVerifyMode: Boolean): IntArray {
    val out = IntArray(sigs.size)
    val dev = sigs.indices.filter { schemes[it].schemeNumberID in GPU_SCHEMES }
    if (dev.isNotEmpty()) {
        val v = gpu.get().verify(CordaGpu.pack(dev.map { schemes[it] }, dev.map { keys[it] }, dev.map { sigs[it] },
                dev.map { data[it] }), doVerifyMode)
        for ((j, i) in dev.withIndex()) out[i] = v[j].toInt()
    }
    for (i in sigs.indices) if (schemes[i].schemeNumberID !in GPU_SCHEMES) {
        out[i] = try {
            val ok = if (doVerifyMode) Crypto.doVerify(schemes[i], keys[i], sigs[i], data[i])
                     else Crypto.isValid(schemes[i], keys[i], sigs[i], data[i])
            if (ok) Verdict.ACCEPT else Verdict.REJECT
        } catch (e: SignatureException) { if (doVerifyMode && e.message == "Signature Verification failed!") Verdict.REJECT else Verdict.SIG_MALFORMED
        } catch (e: InvalidKeyException) { Verdict.KEY_INVALID
        } catch (e: IllegalArgumentException) { Verdict.ARG_EMPTY }
    }
    return out
}

/** Batch [Crypto.isValid]: one verdict code per element (ACCEPT = true). */
fun Crypto.isValidBatch(schemes: List<SignatureScheme>, keys: List<PublicKey>, sigs: List<ByteArray>,
                        data: List<ByteArray>): IntArray = verdicts(schemes, keys, sigs, data, doVerifyMode = false)

/** Batch [Crypto.doVerify]: throws exactly what a for-loop over doVerify would throw first. */
fun Crypto.doVerifyBatch(schemes: List<SignatureScheme>, keys: List<PublicKey>, sigs: List<ByteArray>,
                         data: List<ByteArray>): Boolean {
    val v = verdicts(schemes, keys, sigs, data, doVerifyMode = true)
    for (i in v.indices) when (v[i]) {
        Verdict.ACCEPT -> {}
        Verdict.REJECT -> throw SignatureException("Signature Verification failed!")
        Verdict.SIG_MALFORMED -> throw SignatureException("error decoding signature bytes.")
        Verdict.KEY_INVALID -> throw InvalidKeyException("public key cannot be decoded")
        Verdict.ARG_EMPTY -> throw IllegalArgumentException(
                if (sigs[i].isEmpty()) "Signature data is empty!" else "Clear data is empty, nothing to verify!")
        else -> throw IllegalArgumentException("Unsupported key/algorithm for schemeCodeName: ${schemes[i].schemeCodeName}")
    }
    return true
}

/**
 * `keys[i].isValid(contents[i], sigs[i])` for every i (CryptoUtils.kt:63-67): a Boolean per element,
 * or the first exception the loop would meet — IllegalStateException at the first CompositeKey, else
 * Crypto.isValid's own (SignatureException / InvalidKeyException / IllegalArgumentException).
 * Elements past a CompositeKey are never verified, as in the loop.
 */
fun isValidBatch(keys: List<PublicKey>, contents: List<ByteArray>, sigs: List<DigitalSignature>): BooleanArray {
    val stop = keys.indexOfFirst { it is CompositeKey }.let { if (it < 0) keys.size else it }
    val head = keys.subList(0, stop)
    val v = verdicts(head.map { Crypto.findSignatureScheme(it) }, head, sigs.subList(0, stop).map { it.bytes },
            contents.subList(0, stop), doVerifyMode = false)
    for (i in v.indices) when (v[i]) {
        Verdict.ACCEPT, Verdict.REJECT -> {}
        Verdict.KEY_INVALID -> throw InvalidKeyException("public key cannot be decoded")
        Verdict.SIG_MALFORMED -> throw SignatureException("error decoding signature bytes.")
        else -> throw IllegalArgumentException("Unsupported key/algorithm for schemeCodeName: ${Crypto.findSignatureScheme(keys[i]).schemeCodeName}")
    }
    if (stop < keys.size) throw IllegalStateException("Verification of CompositeKey signatures currently not supported.")
    return BooleanArray(v.size) { v[it] == Verdict.ACCEPT }
}

/** `for (s in sigs) s.verify()` (TransactionSignature.kt:20): each under metaData.publicKey over metaData.bytes(). */
fun verifyTransactionSignaturesBatch(sigs: List<TransactionSignature>): Boolean =
        Crypto.doVerifyBatch(sigs.map { Crypto.findSignatureScheme(it.metaData.publicKey) }, sigs.map { it.metaData.publicKey },
                sigs.map { it.signatureData }, sigs.map { it.metaData.bytes() })

/**
 * `Crypto.doVerify(keys[i], sigs[i])` for every i (Crypto.kt:497-501): verification under the PASSED key
 * over metaData.bytes(); the reference builds, but never throws, the key-mismatch exception (:499),
 * so a mismatching key is not rejected by itself here either.
 */
fun Crypto.doVerifyBatch(keys: List<PublicKey>, sigs: List<TransactionSignature>): Boolean =
        doVerifyBatch(keys.map { findSignatureScheme(it) }, keys, sigs.map { it.signatureData }, sigs.map { it.metaData.bytes() })

/**
 * Batch form of TransactionWithSignatures.checkSignaturesAreValid (TransactionWithSignatures.kt:58-62)
 * for many transactions at once: each signature over its tx's id.bytes, first failure wins.
 */
fun checkSignaturesAreValidBatch(txIds: List<ByteArray>, sigsPerTx: List<List<DigitalSignature.WithKey>>) {
    val flat = sigsPerTx.flatten()
    val data = sigsPerTx.withIndex().flatMap { (t, s) -> List(s.size) { txIds[t] } }
    Crypto.doVerifyBatch(flat.map { Crypto.findSignatureScheme(it.by) }, flat.map { it.by }, flat.map { it.bytes }, data)
}

/**
 * `stx.verifySignaturesExcept(*allowed[t])` for every tx (TransactionWithSignatures.kt:41-47) in one
 * device call — the shape FinalityFlow.kt:159-166 and ResolveTransactionsFlow.kt:85-89 loop over.
 * Transactions whose signatures include a non-GPU scheme take the JVM path unchanged.
 */
fun verifySignaturesExceptBatch(stxs: List<SignedTransaction>, allowed: List<Set<PublicKey>>) {
    val (dev, jvm) = stxs.indices.partition { t -> stxs[t].sigs.all { Crypto.findSignatureScheme(it.by).schemeNumberID in GPU_SCHEMES } }
    for (t in jvm) stxs[t].verifySignaturesExcept(*allowed[t].toTypedArray())
    if (dev.isEmpty()) return
    val batch = dev.map { stxs[it] }
    val arena = TxArena.of(batch.map { it.tx }, batch.map { it.sigs.size })
    val flat = batch.flatMap { it.sigs }
    val sigs = CordaGpu.pack(flat.map { Crypto.findSignatureScheme(it.by) }, flat.map { it.by }, flat.map { it.bytes },
            flat.map { ByteArray(0) })
    val (status, missing) = gpu.get().txVerifySignaturesExcept(arena, sigs, RequiredKeys.of(batch, dev.map { allowed[it] }))
    for ((j, st) in status.withIndex()) when {
        st == TxStatus.OK -> {}
        st >= 0 -> batch[j].sigs[st].verify(batch[j].id.bytes)  // rethrows the JVM's own exception for that signature
        st == TxStatus.SIGNATURES_MISSING -> throw SignedTransaction.SignaturesMissingException(
                missing[j].toSet().let { net.corda.core.utilities.NonEmptySet.copyOf(it) }, batch[j].getKeyDescriptions(missing[j].toSet()), batch[j].id)
        else -> batch[j].verifySignaturesExcept(*allowed[dev[j]].toTypedArray())  // NO_SIGNATURES / NO_COMPONENTS: the JVM throws
    }
}

// ---------------------------------------------------------------- signing (Crypto.doSign, Crypto.kt:394-401)
/** `privateKeys.indices.map { Crypto.doSign(privateKeys[it], clearData[it]) }` for Ed25519 keys, one device call. */
fun Crypto.doSignBatch(gpu: CordaGpu, privateKeys: List<EdDSAPrivateKey>, clearData: List<ByteArray>): List<ByteArray> =
        gpu.doSignBatch(privateKeys, clearData)

/**
 * Sketch of the notary's reply path, batched: NotaryFlow.kt:125-126 calls `service.sign(txId.bytes)` per
 * accepted transaction, which NotaryService.kt:75-77 forwards to `keyManagementService.sign(bits, notaryKey)`
 * and that to Crypto.doSign.  A notary that drains its backlog in batches keeps one [CordaGpu.Signer] for its
 * identity key (the key management service hands the private key to the signer once, at start-up) and signs
 * every accepted id of a batch in one call; each result is wrapped exactly as `sign` wraps it.
 */
class NotaryBatchSigner(gpu: CordaGpu, notaryPrivateKey: EdDSAPrivateKey, private val notaryIdentityKey: PublicKey)
    : AutoCloseable {
    private val signer = gpu.Signer(listOf(notaryPrivateKey))

    /** `txIds.map { service.sign(it.bytes) }` */
    fun signBatch(txIds: List<SecureHash>): List<DigitalSignature.WithKey> =
            signer.sign(txIds.map { it.bytes }).map { DigitalSignature.WithKey(notaryIdentityKey, it) }

    override fun close() = signer.close()
}

// ---------------------------------------------------------------- tear-offs (wtx.buildFilteredTransaction)
/**
 * Batch form of `wtxs.map { it.buildFilteredTransaction(filtering) }` — what NotaryFlow.Client does once
 * per notarisation before it sends to a non-validating notary (NotaryFlow.kt:72:
 * `stx.tx.buildFilteredTransaction { it is StateRef || it is TimeWindow }`) and an oracle client in
 * RatesFixFlow.kt:65.  The predicate runs on the JVM, once per component, and only produces the include
 * mask; the privacy salt (last of availableComponents) is never offered to it, as filterWithFun never
 * offers it (WireTransaction.kt:108-117).  Returns, per tx, what buildMerkleTransaction assembles:
 * the root hash, the indices of the visible components with their nonces, and the PartialMerkleTree.
 * FilteredTransaction's constructor is private (MerkleTransaction.kt:147), so the last step —
 * `FilteredTransaction(rootHash, wtx.filterWithFun(filtering) with these nonces, pmt)` — belongs in a
 * companion function next to buildMerkleTransaction (INTEGRATION.md).
 */
class TearOff(val rootHash: SecureHash, val visible: List<Int>, val nonces: List<SecureHash>, val partialMerkleTree: PartialMerkleTree)

fun buildFilteredTransactionsBatch(gpu: CordaGpu, wtxs: List<WireTransaction>, filtering: (Any) -> Boolean): List<TearOff> {
    val arena = TxArena.of(wtxs, wtxs.map { 0 })
    val include = direct(arena.compStart.getInt(4 * wtxs.size))
    var c = 0
    for (w in wtxs) {
        val comps = w.availableComponents
        for ((i, x) in comps.withIndex()) include.put(c++, if (i < comps.size - 1 && filtering(x)) 1 else 0)
    }
    val out = gpu.buildFilteredBatch(arena, include)
    return wtxs.indices.map { t -> TearOff(out.rootHash(t), out.visible(t, arena.compStart), out.nonces(t), out.partialMerkleTree(t)) }
}
