/*
 * include/lachain_bls.h — C ABI of liblachain_bls.so, the MI355X (gfx950) replacement for the native
 * BLS12-381 library behind Lachain's threshold-crypto hot path.
 *
 * Boundary being replaced: Lachain.Crypto (C#) P/Invokes herumi mcl through the NuGet packages
 * MCL.BLS12_381.Net 0.0.4 / MCL.BLS12_381.Native 0.0.5
 * (/root/reference/src/Lachain.Crypto/Lachain.Crypto.csproj:18-19).  That wrapper's sources are not in
 * the reference tree; the export set below is mcl's public C API (mcl/bn.h, mclbn384_256 build) as
 * inferred from the managed call sites (census in SURVEY.md §8b), so the managed wrapper can be
 * re-pointed at this library by changing its DllImport name.  Every function cites the Lachain call
 * site(s) it serves.  The lcb_* functions are the batch entry points the consensus layer (or a shim,
 * INTEGRATION.md) calls with whole batches of shares.
 *
 * Data layouts: the in-memory structs are byte-compatible with mcl's: Montgomery form, 64-bit limbs
 * little-endian (Fr: R = 2^256, Fp: R = 2^384), G1/G2 Jacobian (x, y, z), GT = Fp12 as 12 Fp.
 * All-zero bytes = zero / point at infinity.  Serialized sizes: Fr 32 B, G1 48 B, G2 96 B, GT 576 B
 * (mcl serialize format; pinned by test/Lachain.CryptoTest/SerializationTest.cs).
 *
 * Errors never cross the ABI as exceptions: int functions return 0 on success and -1 on failure,
 * (de)serializers return the number of bytes written/read or 0.  All arithmetic runs on the GPU; if no
 * gfx950 device can be opened, mclBn_init returns -1 and every other call fails loudly (there is no
 * CPU fallback).
 *
 * Threading (callers: one thread per consensus protocol, src/Lachain.Consensus/AbstractProtocol.cs:46-47):
 * every entry point may be called concurrently from any number of threads.  Single-element mcl operations are
 * synchronous and serialized by an internal lock.  Batch calls run in an execution context (lcb_ctx) that owns
 * their device workspaces: the lcb_ctx_* forms take one explicitly, the other forms use the calling thread's
 * own implicit context (one for the *_dev entry points, another for the synchronous host-pointer ones).  Work
 * of one context runs in the order it was enqueued whatever stream it is enqueued on, TPKE and threshold-
 * signature workspaces are separate, and a *_prepared call fails unless its batch shape is the one prepared
 * in the same context.  lcb_set_device applies to every calling thread.
 */
#ifndef LACHAIN_BLS_H
#define LACHAIN_BLS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MCL_BLS12_381 5
#define MCLBN_COMPILED_TIME_VAR 46 /* mclbn384_256: (MCLBN_FP_UNIT_SIZE * 10 + MCLBN_FR_UNIT_SIZE) */

typedef int64_t mclInt;
typedef size_t mclSize;
typedef struct { uint64_t d[4]; } mclBnFr;
typedef struct { uint64_t d[6]; } mclBnFp;
typedef struct { mclBnFp d[2]; } mclBnFp2;
typedef struct { mclBnFp x, y, z; } mclBnG1;
typedef struct { mclBnFp2 x, y, z; } mclBnG2;
typedef struct { mclBnFp d[12]; } mclBnGT;

/* ------------------------------------------------------------------ init / sizes
   Mcl.Init / static constructor of the managed wrapper (dead test/ToolsTest.cs:18 shows `Mcl.Init()`) */
int mclBn_init(int curve, int compiledTimeVar);
int mclBn_getOpUnitSize(void);
int mclBn_getG1ByteSize(void); /* G1.ByteSize = 48 (src/Lachain.Utility/Serialization/SerialiaztionUtils.cs:24-26) */
int mclBn_getFrByteSize(void); /* Fr.ByteSize = 32 */
int mclBn_getFpByteSize(void);

/* ------------------------------------------------------------------ Fr
   Fr.FromInt (23 call sites, e.g. TPKE/PublicKey.cs:79), Fr.GetRandom (TPKE/PublicKey.cs:29),
   Fr.FromBytes / ToBytes (ThresholdSignature/PrivateKeyShare.cs:31), operators + * (MclTests.cs:57) */
int mclBnFr_setInt(mclBnFr *y, mclInt x);
int mclBnFr_setInt32(mclBnFr *y, int x);
int mclBnFr_setByCSPRNG(mclBnFr *x);
int mclBnFr_setLittleEndian(mclBnFr *x, const void *buf, mclSize bufSize);
mclSize mclBnFr_serialize(void *buf, mclSize maxBufSize, const mclBnFr *x);
mclSize mclBnFr_deserialize(mclBnFr *x, const void *buf, mclSize bufSize);
void mclBnFr_clear(mclBnFr *x);
int mclBnFr_isValid(const mclBnFr *x);
int mclBnFr_isEqual(const mclBnFr *x, const mclBnFr *y);
int mclBnFr_isZero(const mclBnFr *x);
int mclBnFr_isOne(const mclBnFr *x);
void mclBnFr_neg(mclBnFr *y, const mclBnFr *x);
void mclBnFr_inv(mclBnFr *y, const mclBnFr *x);
void mclBnFr_sqr(mclBnFr *y, const mclBnFr *x);
void mclBnFr_add(mclBnFr *z, const mclBnFr *x, const mclBnFr *y);
void mclBnFr_sub(mclBnFr *z, const mclBnFr *x, const mclBnFr *y);
void mclBnFr_mul(mclBnFr *z, const mclBnFr *x, const mclBnFr *y);
void mclBnFr_div(mclBnFr *z, const mclBnFr *x, const mclBnFr *y);

/* ------------------------------------------------------------------ G1
   G1.Generator (24 sites), G1.FromBytes (HoneyBadger decode, TPKE/PublicKey.cs:41), G1 * Fr
   (TPKE/PublicKey.cs:30-32, TPKE/PrivateKey.cs:28), G1 + G1 (MclTests.cs:59), IsValid
   (ThresholdKeygen/Data/Commitment.cs:78) */
mclSize mclBnG1_serialize(void *buf, mclSize maxBufSize, const mclBnG1 *x);
mclSize mclBnG1_deserialize(mclBnG1 *x, const void *buf, mclSize bufSize);
int mclBnG1_isValid(const mclBnG1 *x);
int mclBnG1_isEqual(const mclBnG1 *x, const mclBnG1 *y);
int mclBnG1_isZero(const mclBnG1 *x);
void mclBnG1_clear(mclBnG1 *x);
void mclBnG1_neg(mclBnG1 *y, const mclBnG1 *x);
void mclBnG1_dbl(mclBnG1 *y, const mclBnG1 *x);
void mclBnG1_normalize(mclBnG1 *y, const mclBnG1 *x);
void mclBnG1_add(mclBnG1 *z, const mclBnG1 *x, const mclBnG1 *y);
void mclBnG1_sub(mclBnG1 *z, const mclBnG1 *x, const mclBnG1 *y);
void mclBnG1_mul(mclBnG1 *z, const mclBnG1 *x, const mclBnFr *y);
void mclBnG1_mulVec(mclBnG1 *z, const mclBnG1 *x, const mclBnFr *y, mclSize n);
/* convenience (not in mcl): the Lachain G1 generator (SerializationTest.cs:36) */
void lcb_g1_generator(mclBnG1 *g);

/* ------------------------------------------------------------------ G2
   G2.Generator, G2.FromBytes (ThresholdSignature/Signature.cs:38), G2.SetHashOf
   (TPKE/Utils.cs:24-25, ThresholdSignature/PublicKey.cs:19, PrivateKeyShare.cs:24), G2 * Fr
   (TPKE/PublicKey.cs:34, PrivateKeyShare.cs:25) */
mclSize mclBnG2_serialize(void *buf, mclSize maxBufSize, const mclBnG2 *x);
mclSize mclBnG2_deserialize(mclBnG2 *x, const void *buf, mclSize bufSize);
int mclBnG2_isValid(const mclBnG2 *x);
int mclBnG2_isEqual(const mclBnG2 *x, const mclBnG2 *y);
int mclBnG2_isZero(const mclBnG2 *x);
void mclBnG2_clear(mclBnG2 *x);
int mclBnG2_hashAndMapTo(mclBnG2 *x, const void *buf, mclSize bufSize);
void mclBnG2_neg(mclBnG2 *y, const mclBnG2 *x);
void mclBnG2_dbl(mclBnG2 *y, const mclBnG2 *x);
void mclBnG2_normalize(mclBnG2 *y, const mclBnG2 *x);
void mclBnG2_add(mclBnG2 *z, const mclBnG2 *x, const mclBnG2 *y);
void mclBnG2_sub(mclBnG2 *z, const mclBnG2 *x, const mclBnG2 *y);
void mclBnG2_mul(mclBnG2 *z, const mclBnG2 *x, const mclBnFr *y);
void lcb_g2_generator(mclBnG2 *g);

/* ------------------------------------------------------------------ GT / pairing
   GT.Pairing (8 sites: TPKE/PrivateKey.cs:26, TPKE/PublicKey.cs:91, ThresholdSignature/PublicKey.cs:20),
   GT.Equals, GT.Pow (MclTests.cs:73) */
void mclBn_pairing(mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y);
void mclBn_millerLoop(mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y);
void mclBn_millerLoopVec(mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y, mclSize n);
void mclBn_finalExp(mclBnGT *y, const mclBnGT *x);
int mclBnGT_isEqual(const mclBnGT *x, const mclBnGT *y);
int mclBnGT_isOne(const mclBnGT *x);
int mclBnGT_isZero(const mclBnGT *x);
void mclBnGT_clear(mclBnGT *x);
void mclBnGT_mul(mclBnGT *z, const mclBnGT *x, const mclBnGT *y);
void mclBnGT_pow(mclBnGT *z, const mclBnGT *x, const mclBnFr *y);
mclSize mclBnGT_serialize(void *buf, mclSize maxBufSize, const mclBnGT *x);
mclSize mclBnGT_deserialize(mclBnGT *x, const void *buf, mclSize bufSize);

/* ------------------------------------------------------------------ polynomials / Lagrange
   MclBls12381.LagrangeInterpolate (TPKE/PublicKey.cs:83, ThresholdSignature/PublicKeySet.cs:31,41,
   ThresholdKeygen/Data/State.cs:43), MclBls12381.EvaluatePolynomial (TPKE/TrustedKeyGen.cs:23-33) */
int mclBn_FrLagrangeInterpolation(mclBnFr *out, const mclBnFr *xVec, const mclBnFr *yVec, mclSize k);
int mclBn_G1LagrangeInterpolation(mclBnG1 *out, const mclBnFr *xVec, const mclBnG1 *yVec, mclSize k);
int mclBn_G2LagrangeInterpolation(mclBnG2 *out, const mclBnFr *xVec, const mclBnG2 *yVec, mclSize k);
int mclBn_FrEvaluatePolynomial(mclBnFr *out, const mclBnFr *cVec, mclSize cSize, const mclBnFr *x);
int mclBn_G1EvaluatePolynomial(mclBnG1 *out, const mclBnG1 *cVec, mclSize cSize, const mclBnFr *x);
int mclBn_G2EvaluatePolynomial(mclBnG2 *out, const mclBnG2 *cVec, mclSize cSize, const mclBnFr *x);

/* ================================================================== batch entry points (new)
   Host-pointer forms copy to/from the GPU; *_dev forms take device pointers and a hipStream_t (as void*)
   and enqueue without synchronizing.  All serialized inputs use the 48/96-byte wire formats. */

/* library configuration */
int lcb_set_device(int device_id);                 /* before mclBn_init; default: HIP device 0 */
int lcb_get_device(void);
void lcb_set_original_g2_cofactor(int enable);     /* unpinned mcl choice, DESIGN.md §Parity */
/* unpinned mcl convention: the G2 wire flag (bit 7 of byte 95) is the parity of y.a (use_b = 0, the
   default) or of y.b (use_b = 1), for every G2 (de)serialization — the mcl surface and every batch kernel alike.
   Mirrors the oracle's orc_set_g2_sign_from_b (oracle/bls.c:517-521,691).  Call before batch work, not during it.
   Returns -1 without a device. */
int lcb_set_g2_sign_from_b(int use_b);
/* Line sets prepared for TPKE ciphertexts / signed messages are normalised (A = 1) unless a line has A == 0, in
   which case the Miller loop computes that point's lines on the fly.  general = 1 makes every later prepare take
   the on-the-fly path (test hook: the fallback must give the same decisions); 0 restores the default.
   Tuning hook: returns -1 (and changes nothing) unless the environment has LCB_ALLOW_TUNING=1. */
int lcb_set_line_mode(int general);
const char *lcb_last_error(void);
/* number of failures recorded on the calling thread so far (each sets lcb_last_error).  The mcl entry points that
   return void (mclBnG1_mul, mclBn_pairing, ...) have no return code: a caller detects their failure by this counter
   changing across the call.  A failed void call also writes a random, non-canonical value to its output (the top limb
   of the first coordinate is all ones), so two failed calls never compare equal. */
uint64_t lcb_error_count(void);
/* test hook: the next `count` passes through fault site `site` fail (1: the single-operation staging's pinned host
   buffer, 2: the prepared-ciphertext cache's uploads after its slots were assigned, 3: mclBn_pairing, 4: a
   single-operation round trip); 0 disables.  Returns -1 unless the environment has LCB_ALLOW_TEST_HOOKS=1. */
int lcb_test_inject_failure(int site, int count);
/* test hook: the line sets of n G2 wire points (96-byte encodings; an undecodable one is the point at infinity), on the
   five-lane kernel (coop = 1) or the one-lane kernel, force[k] = 1 forcing set k's flag to the on-the-fly path.
   out: n sets of 26,368 bytes (pairing.hpp layout); w_g2[k] = 1 iff point 2k + 1 lies in G2.  Returns -1 unless the
   environment has LCB_ALLOW_TEST_HOOKS=1. */
int lcb_test_linesets(int coop, const uint8_t *g2_wire, const uint8_t *force, size_t n, uint32_t *out, uint8_t *w_g2);

/* TPKE.PublicKey.VerifyShare for a batch (TPKE/PublicKey.cs:88-92, called per share from
   HoneyBadger.cs:211-212).  Ciphertext c = (U_c, V_c, W_c) with V_c = v_data[v_off[c] .. v_off[c+1]);
   share i pairs ciphertext ct_idx[i] with decryptor dec_idx[i] (verification key y_keys[dec_idx[i]]) and
   partial decryption ui[i].  accept[i] = 1 iff e(Ui, H(U||V)) == e(Y_i, W) (malformed encodings -> 0). */
int lcb_tpke_verify_shares(uint8_t *accept, size_t n_shares, const uint8_t *y_keys, size_t n_keys,
                           const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                           const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                           const uint32_t *dec_idx, const uint8_t *ui);
int lcb_tpke_verify_shares_dev(uint8_t *accept, size_t n_shares, const uint8_t *y_keys, size_t n_keys,
                               const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                               const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                               const uint32_t *dec_idx, const uint8_t *ui, void *stream);

/* The two stages of lcb_tpke_verify_shares_dev, for callers that pipeline or time them separately:
   prepare = verification-key decompression + per-ciphertext H(U||V) and Miller-line precomputation into
   the calling thread's TPKE workspace; verify = the per-share pairing-product check against that workspace
   (n_keys and n_cts must be the prepared ones).  The workspace stays valid until the next TPKE prepare in the
   same context (lcb_ctx_* forms below for explicit contexts). */
int lcb_tpke_prepare_dev(const uint8_t *y_keys, size_t n_keys, const uint8_t *cts_u, const uint8_t *cts_w,
                         const uint8_t *v_data, const uint32_t *v_off, size_t n_cts, void *stream);
int lcb_tpke_verify_prepared_dev(uint8_t *accept, size_t n_shares, size_t n_keys, size_t n_cts,
                                 const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui, void *stream);

/* TPKE.PrivateKey.Decrypt for a batch (TPKE/PrivateKey.cs:21-31): status[c] = 1 and ui[c] = x*U_c when
   e(G, W_c) == e(U_c, H(U_c||V_c)), status[c] = 0 ("Invalid share!") otherwise. */
int lcb_tpke_partial_decrypt(uint8_t *ui_out, uint8_t *status, const uint8_t x[32], const uint8_t *cts_u,
                             const uint8_t *cts_w, const uint8_t *v_data, const uint32_t *v_off, size_t n_cts);

/* TPKE.PublicKey.Encrypt for a batch with caller-supplied randomness r (TPKE/PublicKey.cs:25-37):
   U = rG, T = rY (serialized, for the XorWithHash KDF done by the caller), W = r H(U||V). Two-phase
   because V = data XOR KDF(T) is computed between the phases (TPKE/Utils.cs:12-19).  lcb_tpke_encrypt_batch
   ("TPKE keystream on the device" below) is the whole of Encrypt in one call. */
int lcb_tpke_encrypt_phase1(uint8_t *u_out, uint8_t *t_out, const uint8_t y[48], const uint8_t *r, size_t n);
int lcb_tpke_encrypt_phase2(uint8_t *w_out, const uint8_t *u, const uint8_t *r, const uint8_t *v_data,
                            const uint32_t *v_off, size_t n);

/* ThresholdSignature.PublicKey.ValidateSignature for a batch (ThresholdSignature/PublicKey.cs:16-21,
   ThresholdSigner.cs:62,89-92): share i is checked against message msg_idx[i] (messages concatenated in
   msg_data with offsets msg_off) and public key pks[pk_idx[i]].  accept[i] = e(PK, H(m)) == e(G, sig). */
int lcb_ts_verify_shares(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                         const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                         const uint32_t *msg_idx, const uint32_t *pk_idx);
int lcb_ts_verify_shares_dev(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                             const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                             const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream);

/* Split form of lcb_ts_verify_shares_dev for callers that verify several batches against the same messages and
   keys (e.g. the shares of a coin, then the combined signature): prepare decompresses the keys and hashes every
   message to G2 with its Miller lines; verify_prepared checks items against that workspace. */
int lcb_ts_prepare_dev(const uint8_t *pks, size_t n_pks, const uint8_t *msg_data, const uint32_t *msg_off,
                       size_t n_msgs, void *stream);
int lcb_ts_verify_prepared_dev(uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs, const uint8_t *sigs,
                               const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream);
/* ThresholdSigner.AddShare assembly for whole batches of rounds (ThresholdSigner.cs:62-75, PublicKeySet.cs:34-42):
   round r owns shares [r*per_round, (r+1)*per_round) with verification bits in accept (device); the first k
   accepted shares in index order (x = index + 1) are Lagrange-combined in G2.  sig_out: n_rounds x 96 B,
   status[r] = 0 when round r has fewer than k valid shares.  All pointers are device pointers. */
int lcb_ts_assemble_dev(uint8_t *sig_out, uint8_t *status, const uint8_t *accept, const uint8_t *sigs,
                        size_t per_round, size_t k, size_t n_rounds, void *stream);

/* TPKE.PrivateKey.Decrypt (TPKE/PrivateKey.cs:21-31) against the workspace of lcb_tpke_prepare_dev (same
   ciphertexts): ciphertext validity e(G, W) == e(U, H), then U_i = x U.  x_raw: 32-byte LE secrets (device),
   x_stride = 0 uses one secret for every ciphertext, 1 gives ciphertext c its own secret x_raw[c] (one
   decrypting node per ciphertext, as in an epoch replay).  ui_out: 48 B per ciphertext (zero when invalid),
   status[c] = validity.  Device pointers. */
int lcb_tpke_partial_decrypt_prepared_dev(uint8_t *ui_out, uint8_t *status, const uint8_t *x_raw, size_t x_stride,
                                          const uint8_t *cts_u, size_t n_cts, void *stream);
/* TPKE.PublicKey.FullDecrypt's combination step (TPKE/PublicKey.cs:74-84) for whole batches: ciphertext c owns
   shares [c*per_ct, (c+1)*per_ct) ordered by DecryptorId, with verification bits in accept; the first k
   accepted shares (x = DecryptorId + 1) are Lagrange-combined in G1: u_out[c] = sum lambda_i U_i (48 B),
   status[c] = 0 with fewer than k valid shares.  The plaintext is then lcb_xor_with_hash(u, V) on the host
   (lcb_tpke_full_decrypt_dev, "TPKE keystream on the device" below, goes on to the plaintext on the device). */
int lcb_tpke_combine_dev(uint8_t *u_out, uint8_t *status, const uint8_t *accept, const uint8_t *shares,
                         size_t per_ct, size_t k, size_t n_cts, void *stream);
/* Arrival-order forms of the two combinations: HoneyBadger.cs:237-247 / ThresholdSigner.cs:62-75 combine the first
   F+1 valid shares to ARRIVE.  order (device, per_group u32 per group): order[g * per_group + j] = the position
   (DecryptorId / signer index) of the j-th share to arrive in group g; entries >= per_group mark arrivals that did
   not happen.  A position listed twice makes the group fail (status 0: repeated abscissa).  The selection then
   walks this order instead of index order; everything else is as lcb_tpke_combine_dev / lcb_ts_assemble_dev. */
int lcb_tpke_combine_ordered_dev(uint8_t *u_out, uint8_t *status, const uint8_t *accept, const uint8_t *shares,
                                 const uint32_t *order, size_t per_ct, size_t k, size_t n_cts, void *stream);
int lcb_ts_assemble_ordered_dev(uint8_t *sig_out, uint8_t *status, const uint8_t *accept, const uint8_t *sigs,
                                const uint32_t *order, size_t per_round, size_t k, size_t n_rounds, void *stream);

/* device time (ms) of k_tpke_miller and k_final_exp_check in the last split TPKE verify (waits for it) */
int lcb_tpke_verify_phase_ms(float ms[2]);
/* Line sets of up to max_sets points per preparation on the five-lane kernel (latency), larger preparations one lane
   per set (throughput); -1 restores the default (8,192).  Tuning hook: -1 unless LCB_ALLOW_TUNING=1. */
int lcb_set_lines_coop_max(int max_sets);
/* 1 (default): the fused batched calls build the validators' fixed-base tables before forking the preparation streams;
   0: on the randomisation stream beside them.  Tuning hook: -1 unless LCB_ALLOW_TUNING=1. */
int lcb_set_keys_first(int on);
/* The batched TPKE check's exponents.  lcb_set_rlc_share_exponents(1): one independent exponent per share, drawn from
   its index in the batch; 0 (default): one per position in a level-1 group, t[ct_idx & 3][pos], 128 per call.
   lcb_set_rlc_lane_permutation(0): the randomisation's lanes take the shares in batch order; 1 (default): sorted by
   exponent, so that a wave skips the ladder columns its one exponent does not need.  lcb_set_rlc_pos_table_min: with
   position exponents, batches of at least this many shares per key read the keys' multiples from a table of 128 per key
   (default 512; 0: always; UINT32_MAX: never).  lcb_set_rlc_signed_digits(1) (default): a wave that holds one exponent
   walks its Joint Sparse Form (signed digits, about 16.5 additions instead of 24); 0: its binary columns.  The exponents
   and the decisions are the same in every setting.  Tuning hooks: -1 unless LCB_ALLOW_TUNING=1. */
int lcb_set_rlc_share_exponents(int on);
int lcb_set_rlc_lane_permutation(int on);
int lcb_set_rlc_pos_table_min(uint32_t shares_per_key);
int lcb_set_rlc_signed_digits(int on);

/* Randomized batch form of lcb_tpke_verify_prepared_dev (same arguments, same workspace, same validity rules;
   replaces the per-share loop over TPKE/PublicKey.cs:88-92 driven from HoneyBadger.cs:211-212).  Shares are grouped
   into runs of one ciphertext (pass ciphertext-major batches); a group is accepted when
   e(sum r_i U_i, H) == e(sum r_i Y_i, W) for secret 64-bit r_i (getrandom per call), a failed group is split and
   re-checked down to single shares.  Every rejection is exact; a false acceptance has probability <= 2^-64 per group.
   Returns when the decisions are final (one small device-to-host read per splitting level). */
int lcb_tpke_verify_prepared_batched_dev(uint8_t *accept, size_t n_shares, size_t n_keys, size_t n_cts,
                                         const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui,
                                         void *stream);
/* prepare + batched verify in one call (arguments of lcb_tpke_verify_shares_dev): the per-share randomisation runs on
   a second stream of the context beside the per-ciphertext hashing and line sets; the prepared workspace is left as
   lcb_tpke_prepare_dev leaves it */
int lcb_tpke_verify_shares_batched_dev(uint8_t *accept, size_t n_shares, const uint8_t *y_keys, size_t n_keys,
                                       const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                       const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                       const uint32_t *dec_idx, const uint8_t *ui, void *stream);
/* lcb_tpke_verify_shares with a per-context cache of prepared ciphertexts (2048 slots: the line sets of H and W and
   the ciphertext's validity, keyed by its bytes U || W || V, least recently used replaced) and of decompressed
   verification keys (4096 slots).  For callers that verify a ciphertext's shares over several calls
   (HoneyBadger.cs:211-212 verifies one share per call): each ciphertext is hashed to G2 and its Miller lines computed
   once.  A call with more than 1024 ciphertexts or more than 4096 keys runs uncached.  Same decisions as
   lcb_tpke_verify_shares for any input. */
int lcb_tpke_verify_shares_cached(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                  const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                  const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx, const uint32_t *dec_idx,
                                  const uint8_t *ui);
/* host-pointer form of the batched verify (arguments of lcb_tpke_verify_shares) */
int lcb_tpke_verify_shares_batched(uint8_t *accept, size_t n_shares, const uint8_t *y_keys, size_t n_keys,
                                   const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                   const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                   const uint32_t *dec_idx, const uint8_t *ui);
/* Randomized batch forms of the threshold-signature share check (ThresholdSignature/PublicKey.cs:16-21, called per
   share from ThresholdSigner.cs:62): groups = runs of shares of one message (pass message-major batches), checked as
   e(sum s_i PK_i, H(m)) == e(G, sum s_i sig_i); a share whose signature is outside G2 gets its exact check.  Same
   arguments as lcb_ts_verify_prepared_dev / lcb_ts_verify_shares_dev / lcb_ts_verify_shares. */
int lcb_ts_verify_prepared_batched_dev(uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs, const uint8_t *sigs,
                                       const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream);
int lcb_ts_verify_shares_batched_dev(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                                     const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                                     const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream);
int lcb_ts_verify_shares_batched(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                                 const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                                 const uint32_t *msg_idx, const uint32_t *pk_idx);
/* the last batched verify (TPKE or threshold signatures) completed by the calling thread (any context; the
   lcb_ctx_ form: the last one of that context): groups checked per level
   (levels[0] = level 1, levels[1] = the level-2 weighted re-checks of failed groups, then single checks) and device
   ms of [randomisation + grouping, all levels, then summed over the levels: group sums, group Miller loops, final
   exponentiations (+ resolve / search), the fused call's preparation chain (hashing, line sets and census on the
   preparation stream, beside the randomisation; 0 for other calls)]; returns the number of levels (waits for the call) */
int lcb_tpke_batched_stats(uint32_t levels[8], float ms[6]);
/* test hook: fixed 32-byte ChaCha20 key for the batch exponents (NULL restores getrandom).  Honoured only when the
   environment has LCB_ALLOW_FIXED_BATCH_SEED=1 (a fixed key makes the exponents predictable); ignored otherwise. */
void lcb_set_batch_seed(const uint8_t *seed32);
/* Byzantine validators (HoneyBadgerMalicious.cs:17-23 corrupts the share a faulty validator sends in EVERY
   ciphertext): batched calls of at least min_shares shares (default 16384; 0 = never) first check a prefix of the
   batch (512..2048 shares, at most a quarter) share by share — the census — and mark a key suspect when at least half
   of its sampled, decodable shares failed; every share of a suspect key is then checked on its own and the groups are
   summed over the other keys.  Decisions are unchanged; only the cost changes. */
void lcb_set_batch_census(size_t min_shares);
/* census of the last batched verify: {census shares, suspect keys, level-1 groups, level-1 entries after moving the
   suspect keys' shares to single checks} (lcb_ctx_ form: that context's last one) */
int lcb_batched_census(uint32_t out[4]);
/* levels of at most max_checks group checks run on the cooperative kernels (k_coop.hip: nine lanes per pairing check,
   lower latency below one wave per SIMD); 0 = always one check per lane.  Default 32768.  This and the next two are
   tuning hooks: each returns -1 (and changes nothing) unless the environment has LCB_ALLOW_TUNING=1. */
int lcb_set_coop_max(uint32_t max_checks);
/* the cooperative threshold of the group Miller loops alone (default 65536; the final exponentiations keep
   lcb_set_coop_max's) */
int lcb_set_coop_miller_max(uint32_t max_checks);
/* level 1 of the TPKE batched check: chunks of at least min_entries entries run one final exponentiation per pair of
   randomized groups (a second pass exponentiates one member of each pair that failed; the other's value is the
   quotient), instead of one per group.  0 = never; UINT32_MAX (the default) = more entries than lcb_set_coop_max's
   value.  Decisions are unchanged.  Tuning hook (LCB_ALLOW_TUNING=1). */
int lcb_set_fe_pair_min(uint32_t min_entries);
/* that stage in the calling thread's last batched verify (lcb_ctx_ form: that context's last one): {pairs formed,
   pairs that failed, final exponentiations run in pass 1, in pass 2}; all 0 when the stage did not run */
int lcb_tpke_fe_pair_stats(uint32_t out[4]);
/* The final exponentiation of a TPKE level when batches overlap.  The library counts, per device, the batched TPKE
   verify calls (lcb_tpke_verify_shares_batched, its _dev and lcb_ctx_ forms) between entry and return.  A call that
   sees at least one other call counted on its device when it enqueues a level's final exponentiation (a single pass,
   either pass of the pair stage, any level) runs it on the nine-lane kernel only if the dispatch has at most
   max_checks checks, otherwise on the one-lane kernel, which issues about a third fewer instructions per check; a
   call that has the device to itself keeps lcb_set_coop_max's rule.  UINT32_MAX = the rule is off.  The Miller loops
   (lcb_set_coop_miller_max), the pair stage's trigger (lcb_set_fe_pair_min), CommonCoin and the census are not
   affected.  Keep it at 1024 or more: a one-lane final exponentiation takes about 12 ms however few checks it has,
   and the aggregation queue's workers overlap each other with flushes of at most 64 shares.  Decisions are
   unchanged.  Tuning hook (LCB_ALLOW_TUNING=1). */
int lcb_set_busy_coop_max(uint32_t max_checks);
uint32_t lcb_busy_coop_max(void);          /* the value in force */
/* test / A-B switch of that rule: 0 = by the in-flight count (the default), 1 = never overlapped, 2 = always
   overlapped (every batched TPKE level, the prepared forms included).  Tuning hook (LCB_ALLOW_TUNING=1). */
int lcb_set_level_mode(int mode);
/* batched TPKE verify calls now between entry and return on `device` (-1: device out of range) */
int lcb_batched_inflight(int device);
/* shares / group checks per Miller + final-exponentiation launch pair (default and maximum 2^21): a test hook that
   makes small batches run several chunks (chunk offsets in the copies and searches).  Set it only while no batch call
   is in flight.  Tuning hook (LCB_ALLOW_TUNING=1). */
int lcb_set_verify_chunk(size_t checks);
/* stream layout of the fused batched verifies (lcb_tpke_verify_shares_batched_dev, lcb_ts_verify_shares_batched_dev):
   0 = randomisation on the context's second stream beside the preparation on the caller's; 1 = the
   latency-bound preparation chain (hash-to-G2, line sets, census) on a high-priority stream and the randomisation on
   the caller's; 2 = as 1 with the preparation's first kernel enqueued ahead of the randomisation; 3 = as 2 with the
   TPKE preparation split into hash + H's line set and U / W decoding + W's line set, on two more high-priority
   streams; 4 (default, round 6) = the split preparation's two lane kinds in one dispatch on the one high-priority
   stream, the census behind it, so a context uses one hardware queue per priority (threshold signatures: modes 2-4
   act as 1).  Decisions are unchanged. */
int lcb_set_fork_mode(int mode);
/* the scratch gate (round 6 model): the HSA runtime binds a dispatch's FULL-device scratch
   (private segment per lane rounded to 16 B x 64 lanes x CUs x 32 wave slots) to its hardware queue whenever that is
   below the agent's bind limit (24 GiB on the box), and all queues share one pool (32 GiB); a request the pool cannot
   serve aborts the process.  A launch whose full-device size exceeds the per-queue share T = (pool - 4.5 GiB) / Q
   (Q = 2 x GPU_MAX_HW_QUEUES: the library uses two stream priorities) runs on one process-wide stream per device,
   ordered with the caller's stream by events, so the queues' bound scratch stays within the pool.  `bytes` replaces T
   (environment LCB_SCRATCH_GATE_MB); -1 = off, 0 = every launch with scratch, < -1 = back to the model.  Tuning hook
   (LCB_ALLOW_TUNING=1). */
int lcb_set_scratch_gate(long long bytes);
/* the calling thread's device's scratch model: out[0] pool bytes (HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_MAX, 0 unknown),
   [1] bind limit (..._SCRATCH_LIMIT_CURRENT), [2] wave slots (CUs x waves per CU), [3] Q, [4] the per-queue share T,
   [5] the threshold in force (UINT64_MAX: gate off).  0 on success. */
int lcb_scratch_info(uint64_t out[6]);
/* launches routed through the gate / launches checked, since the process started */
void lcb_scratch_gate_stats(uint64_t *routed, uint64_t *seen);
/* the persistent grids of the table-walking kernels (Lagrange lanes, scalar-multiplication batches) use at most this
   many blocks of 256 lanes (0 = as many as are resident): a test hook that makes small batches walk several items per
   lane.  Tuning hook (LCB_ALLOW_TUNING=1). */
int lcb_set_persist_blocks(uint32_t max_blocks);
/* tuning hook (LCB_ALLOW_TUNING=1): records per lane of the MSM bucket accumulation (k_msm_chunk_acc, default 64);
   0 = one lane per bucket (k_msm_bucket_acc).  Results are unchanged. */
int lcb_set_msm_chunk(int records_per_lane);
/* tuning hook (LCB_ALLOW_TUNING=1): the MSM bucket reduction uses the fewest serial segments up to max_segments lanes
   (0 = by form: the GLV form the fewest segments up to 65,536, the plain form the most of at least 65,536).
   Results are unchanged. */
int lcb_set_msm_segments(int max_segments);
/* tuning hook (LCB_ALLOW_TUNING=1): 1 (default) = the latency-bound kernels of the batched checks (preparation chain,
   every level) raise their waves' issue priority over the bulk randomisation waves sharing their SIMDs; 0 = off */
int lcb_set_wave_priority(int on);
/* test hook: final exponentiation of n Fp12 values (144 x u32 each, Montgomery form, field.hpp layout) by the one-lane
   (coop = 0) or the cooperative (coop = 1) kernel */
int lcb_debug_final_exp(const uint32_t *in, size_t n, uint32_t *out, int coop);
/* test hook: one cooperative Fp12 operation (op: 0 square, 1 cyclotomic square, 2 product, 3 product by the conjugate,
   4..6 Frobenius 1..3, 7 inverse, 8 conjugate, 9 sparse line product, 10 final exponentiation) on n values a (and b),
   with the one-lane field.hpp result beside it in ref */
int lcb_debug_coop_op(int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out, uint32_t *ref);
/* test hook: one routine of the assembly tower on n (1..65536) arbitrary Fp12 operands a (and b), same layout.
   op & 255: 0 a b, 1 conj(a) b, 2 one Granger-Scott squaring, 3 a run of op >> 8 (1..255) squarings in one call,
   4 a^z (z < 0 the curve parameter; a unitary).  b is read by ops 0 and 1 only. */
int lcb_debug_asm_tower(int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out);
/* test hook: one routine of the secp256k1 device code on n (1..65536) arbitrary items, one lane each.  Words are
   little-endian 32-bit limbs of 256-bit values; any value in [0, 2^256) is a legal field operand.
   a and b, 25 words per item: x[8] y[8] z[8] inf.  A field or scalar operand is x; a point is Jacobian (x, y, z) with
   inf != 0 for infinity; the affine operand of op 15 is (x, y) of b.  b may be null for operations of one operand.
   out, 44 words per item: x[8] y[8] z[8] inf flags digits[18].
   op 0..8: field mul, sqr, add, sub, neg, dbl, canon, inv (0 -> 0), sqrt (a^((p+1)/4)) -> x, weakly reduced except canon.
   op 9: flags bit 0 a == 0, bit 1 a odd, bit 2 a == b (all mod p).
   op 10: a b R^-1 mod n, op 11: (a R^-1)^-1 R mod n (R = 2^256; operands below n) -> x.
   op 12: the endomorphism split of a and the signed 4-bit digits of both halves: magnitudes -> x, y; flags bit 0 / 1:
   the first / second half is negative; digits: 36 signed bytes per half, low window first.
   op 13: the comb's signed 8-bit digits of a -> digits, 36 signed bytes.
   op 14: 2 a, op 15: a + affine b, op 16: a + b -> (x, y, z, inf); an infinite result has zero coordinates. */
int lcb_debug_secp_op(int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out);
/* test hook: one routine under G2.SetHashOf, or one device point decoder, on n (1..65536) arbitrary items, one lane each.
   in, 48 words per item; out, 76 words per item: value words [0, 72), out[72] = the routine's flag, out[73] = 1 for a
   decoded point at infinity, the rest zero.  A field operand is 12 little-endian 32-bit words in Montgomery form (m =
   a 2^384 mod p, below p; the convention of lcb_debug_fp12), an Fp2 operand a[12] b[12]; byte strings are packed
   little-endian into the words.
   op 0: fp_sqrt of in[0..12) -> a^((p+1)/4) at [0, 12), flag = it is a root.
   op 1: fp2_sqrt of in[0..24) -> mcl's root at [0, 24), flag = a root exists (zero words without one).
   op 2: fp2_sqrt_any, the same layout: a root of either sign.
   op 3: fp2_sqrt_normed: flag = the norm is a square; then the root (mcl's) at [0, 24), from the norm's root as the
         map forms it; zero words otherwise (the routine is not run on a non-square).
   op 4: fp_inv_gcd of in[0..12) -> [0, 12) (0 -> 0).   op 5: fp2_inv_g of in[0..24) -> [0, 24).
   op 6: Fp::setHashOf's reduction of a 64-byte SHA-512 digest (in[0..16)) -> t at [0, 12).
   op 7: MapTo::calcBN of t = in[0..24) -> affine x at [0, 24), y at [24, 48), flag = a point was found.
   op 8: the Budroni-Pintore cofactor clearing, op 9: multiplication by the original cofactor h2, of the affine twist
         point x = in[0..24), y = in[24..48) -> Jacobian (X, Y, Z) at [0, 72); Z = 0 is the point at infinity.
   op 10: the device G1 decoder on 48 bytes -> affine x at [0, 12), y at [12, 24); op 11: the device G2 decoder on 96
          bytes -> x at [0, 24), y at [24, 48); flag = accepted, out[73] = infinity (zero coordinates).
   op 12: mclBnG2_hashAndMapTo's second kernel (the four-lane cofactor clearing) alone, once per item, on the mapped
          point (x, y, 1) given as for op 8 -> Jacobian at [0, 72), flag = 1. */
int lcb_debug_h2g2_op(int op, const uint32_t *in, size_t n, uint32_t *out);
/* test hook: lcb_tpke_verify_shares up to its Miller loop (the one-lane kernel) for n (1..65536) shares, without the
   final exponentiation: f_out = each share's Miller value (144 x u32), ok_out = its validity flag */
int lcb_debug_tpke_miller(uint32_t *f_out, uint8_t *ok_out, size_t n, const uint8_t *y_keys, size_t n_keys,
                          const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data, const uint32_t *v_off,
                          size_t n_cts, const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui);
/* The two test hooks of the batched checks' random exponents.  A share's exponent is a + b lambda,
   lambda = z^2 - 1, with (a, b) words 0 and 1 of the ChaCha20 block (RFC 8439) whose key is the call's 32 getrandom
   bytes and whose words 12..15 are counter, domain, nonce low, nonce high; (0, 0) reads as (1, 0).  Both return -1
   unless the environment has LCB_ALLOW_TEST_HOOKS=1: with a secret key they would expose material of the exponents.
   lcb_debug_rlc_scalars: the device routine that draws (a, b), on n (1..65536) arbitrary items, one lane each.
   key10[10 i ..] = item i's eight key words and two nonce words, ctr[i] / dom[i] its counter and domain;
   ab_out[2 i], ab_out[2 i + 1] = its (a, b). */
int lcb_debug_rlc_scalars(const uint32_t *key10, const uint32_t *ctr, const uint32_t *dom, size_t n, uint32_t *ab_out);
/* lcb_debug_rlc_records: after a batched TPKE or threshold-signature call on ctx (NULL: the calling thread's implicit
   context of the *_dev forms), waits for the context's work and returns the two multiples the call's randomisation
   stored for each of its n shares, as wire bytes (infinity: zero bytes; a share the call left out of its groups, or a
   share of the census prefix, has two points at infinity).
   After a TPKE call (*kind = 0): rec_a[48 i ..] = a U_i + b phi(U_i), rec_b[48 i ..] = a Y + b phi(Y) for the share's
   point U_i and its decryptor's key Y, phi(x, y) = (beta x, y); (a, b) is drawn with counter = the share's bin
   32 (ct_idx & 3) + (its offset in its run of equal ct_idx) mod 32 and domain 1, or, under
   lcb_set_rlc_share_exponents(1), counter = i and domain 0.
   After a threshold-signature call (*kind = 1): rec_a[48 i ..] = a PK + b phi(PK), rec_b[96 i ..] = a S_i + b psi^4(S_i)
   (96 bytes per share), counter = i, domain 0.
   *nonce = the call's nonce: the number of batched calls the context has made, this one included.
   n must equal the last call's share count; -1 otherwise, and when the context has made no batched call. */
struct lcb_ctx;
int lcb_debug_rlc_records(struct lcb_ctx *ctx, uint8_t *rec_a, uint8_t *rec_b, size_t n, uint64_t *nonce, int *kind);

/* ------------------------------------------------------------------ explicit execution contexts
   A context owns the device workspaces of the prepare/verify, assembly, Lagrange and MSM calls below
   (the context-less forms above use the calling thread's implicit context).  ctx == NULL selects that implicit
   context.  A context may be shared by threads (calls on it are serialized) and its work executes in enqueue
   order across streams; lcb_ctx_synchronize waits for all of it. */
typedef struct lcb_ctx lcb_ctx;
lcb_ctx *lcb_ctx_create(void);
void lcb_ctx_destroy(lcb_ctx *ctx);
int lcb_ctx_synchronize(lcb_ctx *ctx);
int lcb_ctx_tpke_prepare_dev(lcb_ctx *ctx, const uint8_t *y_keys, size_t n_keys, const uint8_t *cts_u,
                             const uint8_t *cts_w, const uint8_t *v_data, const uint32_t *v_off, size_t n_cts,
                             void *stream);
int lcb_ctx_tpke_verify_prepared_dev(lcb_ctx *ctx, uint8_t *accept, size_t n_shares, size_t n_keys, size_t n_cts,
                                     const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui, void *stream);
int lcb_ctx_tpke_partial_decrypt_prepared_dev(lcb_ctx *ctx, uint8_t *ui_out, uint8_t *status, const uint8_t *x_raw,
                                              size_t x_stride, const uint8_t *cts_u, size_t n_cts, void *stream);
int lcb_ctx_tpke_combine_dev(lcb_ctx *ctx, uint8_t *u_out, uint8_t *status, const uint8_t *accept,
                             const uint8_t *shares, size_t per_ct, size_t k, size_t n_cts, void *stream);
int lcb_ctx_tpke_combine_ordered_dev(lcb_ctx *ctx, uint8_t *u_out, uint8_t *status, const uint8_t *accept,
                                     const uint8_t *shares, const uint32_t *order, size_t per_ct, size_t k,
                                     size_t n_cts, void *stream);
int lcb_ctx_ts_assemble_ordered_dev(lcb_ctx *ctx, uint8_t *sig_out, uint8_t *status, const uint8_t *accept,
                                    const uint8_t *sigs, const uint32_t *order, size_t per_round, size_t k,
                                    size_t n_rounds, void *stream);
int lcb_ctx_tpke_verify_phase_ms(lcb_ctx *ctx, float ms[2]);
int lcb_ctx_tpke_verify_prepared_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n_shares, size_t n_keys,
                                             size_t n_cts, const uint32_t *ct_idx, const uint32_t *dec_idx,
                                             const uint8_t *ui, void *stream);
int lcb_ctx_tpke_verify_shares_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n_shares, const uint8_t *y_keys,
                                           size_t n_keys, const uint8_t *cts_u, const uint8_t *cts_w,
                                           const uint8_t *v_data, const uint32_t *v_off, size_t n_cts,
                                           const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui,
                                           void *stream);
int lcb_ctx_tpke_batched_stats(lcb_ctx *ctx, uint32_t levels[8], float ms[6]);
int lcb_ctx_batched_census(lcb_ctx *ctx, uint32_t out[4]);
int lcb_ctx_tpke_fe_pair_stats(lcb_ctx *ctx, uint32_t out[4]);
/* the level final exponentiations of the context's last batched verify (ctx NULL: the default context): {dispatches on
   the one-lane kernel, on the nine-lane kernel, one-lane dispatches taken because the call was overlapped
   (lcb_set_busy_coop_max), the largest in-flight count seen when a TPKE level chose}; the census is not counted */
int lcb_ctx_tpke_level_kernel_stats(lcb_ctx *ctx, uint32_t out[4]);
int lcb_ctx_ts_verify_prepared_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs,
                                           const uint8_t *sigs, const uint32_t *msg_idx, const uint32_t *pk_idx,
                                           void *stream);
int lcb_ctx_ts_verify_shares_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks,
                                         const uint8_t *sigs, const uint8_t *msg_data, const uint32_t *msg_off,
                                         size_t n_msgs, const uint32_t *msg_idx, const uint32_t *pk_idx,
                                         void *stream);
int lcb_ctx_ts_prepare_dev(lcb_ctx *ctx, const uint8_t *pks, size_t n_pks, const uint8_t *msg_data,
                           const uint32_t *msg_off, size_t n_msgs, void *stream);
int lcb_ctx_ts_verify_prepared_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs,
                                   const uint8_t *sigs, const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream);
int lcb_ctx_ts_assemble_dev(lcb_ctx *ctx, uint8_t *sig_out, uint8_t *status, const uint8_t *accept,
                            const uint8_t *sigs, size_t per_round, size_t k, size_t n_rounds, void *stream);
int lcb_ctx_g1_lagrange_dev(lcb_ctx *ctx, uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                            const uint32_t *off, size_t n_problems, size_t n_entries, void *stream);
int lcb_ctx_g2_lagrange_dev(lcb_ctx *ctx, uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                            const uint32_t *off, size_t n_problems, size_t n_entries, void *stream);
int lcb_ctx_g1_msm_dev(lcb_ctx *ctx, void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n,
                       int window_bits, void *stream);
int lcb_ctx_g1_msm_phase_ms(lcb_ctx *ctx, float *ms, int n_phases);

/* ------------------------------------------------------------------ trustless DKG G1 work
   coeffs: n_comm commitments x (degree+1)(degree+2)/2 serialized G1 coefficients each, in Commitment's symmetric
   Index(i, j) order (src/Lachain.Consensus/ThresholdKeygen/Data/Commitment.cs:14-21,55-59).
   lcb_dkg_commitment_eval: out[q] = Commitment.Evaluate(xs[q], ys[q]) of commitment comm_idx[q] (Commitment.cs:23-37,
     the per-value check of TrustlessKeygen.HandleSendValue, TrustlessKeygen.cs:150-152).
   lcb_dkg_commitment_rows: rows_out[q] = Commitment.Evaluate(xs[q]) = degree+1 points (Commitment.cs:39-53; the
     commit check of HandleCommit, TrustlessKeygen.cs:90-94, and TryGetKeys' Evaluate(0), :166).
   lcb_g1_eval_poly_batch: MclBls12381.EvaluatePolynomial over G1 at many small x (TryGetKeys, TrustlessKeygen.cs:172-174).
   x, y are the reference's int arguments (player indices); status[q] = 0 for a malformed coefficient or a
   comm_idx >= n_comm.  Results equal the reference's Fr-power sums for coefficients in G1. */
int lcb_dkg_commitment_eval(uint8_t *out, uint8_t *status, const uint8_t *coeffs, size_t n_comm, int degree,
                            const uint32_t *comm_idx, const int32_t *xs, const int32_t *ys, size_t n_queries);
int lcb_dkg_commitment_rows(uint8_t *rows_out, uint8_t *status, const uint8_t *coeffs, size_t n_comm, int degree,
                            const uint32_t *comm_idx, const int32_t *xs, size_t n_queries);
int lcb_g1_eval_poly_batch(uint8_t *out, uint8_t *status, const uint8_t *coeffs, size_t n_coeffs, const int32_t *xs,
                           size_t n_points);

/* ------------------------------------------------------------------ reliable broadcast: Reed-Solomon
   The EncryptedShare bytes travel as N shards of a GF(2^8) Reed-Solomon code (polynomial 0x11D, alpha = 2, generator
   roots alpha^0..alpha^(erasures-1): ErasureCoding.cs:13), erasures = 2F.
   lcb_rs_encode = ReliableBroadcast.ErasureCodingShards(input, n_shards, erasures) (ReliableBroadcast.cs:393-419):
     input_len must be a multiple of n_shards - erasures (AugmentInput pads it); shards_out = n_shards x shard bytes.
   lcb_rs_decode = DecodeFromEchos (ReliableBroadcast.cs:421-446): exactly n_shards - erasures echoes, echo e is shard
     from[e]; out = all n_shards shards.  -1 on bad arguments or an unsolvable erasure set (only with > 255 shards). */
int lcb_rs_encode(uint8_t *shards_out, const uint8_t *input, size_t input_len, int n_shards, int erasures);
int lcb_rs_decode(uint8_t *out, const uint8_t *echo_data, const int32_t *from, int n_echos, size_t shard_size,
                  int n_shards, int erasures);

/* ------------------------------------------------------------------ reliable broadcast: Merkle layer
   Every shard travels with a Keccak-256 Merkle proof (original padding, as lcb_keccak256_batch).  The tree of an
   instance with n shards is a heap of 2T 32-byte nodes, T the smallest power of two >= n (ReliableBroadcast.cs:41-43,
   375-386): tree[T + i] = Keccak(shard i), zero bytes for n <= i < T, tree[i] = Keccak(tree[2i] || tree[2i + 1]), root
   tree[1], node 0 zero.  The proof of shard i is tree[((i + T) >> j) ^ 1], j = 0 .. depth - 1, depth = log2 T
   (MerkleTreeBranch, :366-373).  1 <= n <= 256; f is the reference's F (2f parity shards, f = 0: none); offsets are
   uint64 with one entry more than items, in bytes unless stated; batches are many instances of one (n, f) per call.
   lcb_rbc_shard_size: AugmentInput's shard size ceil((payload_len + 4) / (n - 2f)) (:311-319), 0 on bad arguments;
     lcb_rbc_tree_depth: log2 T, -1 on bad arguments.  Both are host arithmetic and need no device.
   lcb_rbc_val_batch = HandleInputMessage's AugmentInput + ConstructValMessages (:116, :321-338) for B payloads
     (payload b = payloads[payload_off[b] .. payload_off[b + 1])): shards_out = n * S_b bytes per instance in instance
     order, roots_out = B x 32, proofs_out = B x n x depth x 32.  Each output may be null.
   lcb_rbc_check_echo_* = CheckEchoMessage (:296-309) per item: accept[t] = 1 iff the walk from Keccak(data_t) at leaf
     from[t] over the item's proof hashes proofs[proof_off[t] .. proof_off[t + 1]) (offsets in hashes) ends at the root
     with roots[t]; a proof shorter than the depth rejects, entries beyond it are ignored, from outside [0, n) rejects.
   lcb_rbc_merkle_tree_* = ConstructMerkleTree for shards the caller holds (instance b: n_shards equal shards in
     shards[shard_off[b] .. shard_off[b + 1])): trees_out = B x 2T x 32 (8-byte aligned in the device forms).
   lcb_rbc_decode_batch = TrySendReadyMessageFromEchos' work (:201-234): exactly n - 2f echoes per instance in any order
     (instance b's echoes concatenated in echo_data[echo_off[b] .. echo_off[b + 1]), echo e of it is shard
     from[b * (n - 2f) + e]); shards_out as lcb_rs_decode gives them, roots_out the rebuilt tree's root, root_ok[b] =
     (status[b] and rebuilt == expected_roots[b]); expected_roots / root_ok / roots_out / shards_out may be null.  A
     duplicate or out-of-range index or an unsolvable erasure set gives status[b] = 0 and zero output for that instance
     alone.
   The *_dev forms take device pointers and are asynchronous on `stream`; they trust the caller's offsets. */
size_t lcb_rbc_shard_size(size_t payload_len, int n, int f);
int lcb_rbc_tree_depth(int n);
int lcb_rbc_val_batch(uint8_t *shards_out, uint8_t *roots_out, uint8_t *proofs_out, const uint8_t *payloads,
                      const uint64_t *payload_off, size_t n_instances, int n, int f);
int lcb_rbc_check_echo_batch(uint8_t *accept, const uint8_t *data, const uint64_t *data_off, const int32_t *from,
                             const uint8_t *roots, const uint8_t *proofs, const uint64_t *proof_off, size_t n_items,
                             int n_shards);
int lcb_ctx_rbc_check_echo_dev(lcb_ctx *ctx, uint8_t *accept, const uint8_t *data, const uint64_t *data_off,
                               const int32_t *from, const uint8_t *roots, const uint8_t *proofs,
                               const uint64_t *proof_off, size_t n_items, int n_shards, void *stream);
int lcb_rbc_check_echo_dev(uint8_t *accept, const uint8_t *data, const uint64_t *data_off, const int32_t *from,
                           const uint8_t *roots, const uint8_t *proofs, const uint64_t *proof_off, size_t n_items,
                           int n_shards, void *stream);
int lcb_rbc_merkle_tree_batch(uint8_t *trees_out, const uint8_t *shards, const uint64_t *shard_off, size_t n_instances,
                              int n_shards);
int lcb_ctx_rbc_merkle_tree_dev(lcb_ctx *ctx, uint8_t *trees_out, const uint8_t *shards, const uint64_t *shard_off,
                                size_t n_instances, int n_shards, void *stream);
int lcb_rbc_merkle_tree_dev(uint8_t *trees_out, const uint8_t *shards, const uint64_t *shard_off, size_t n_instances,
                            int n_shards, void *stream);
int lcb_rbc_decode_batch(uint8_t *shards_out, uint8_t *status, uint8_t *root_ok, uint8_t *roots_out,
                         const uint8_t *echo_data, const uint64_t *echo_off, const int32_t *from,
                         const uint8_t *expected_roots, size_t n_instances, int n, int f);
/* MerkleTree.ComputeRoot (MerkleTree.cs:139-191; the block's transaction root checked in BlockManager.cs:692): tree t is
   hashes[off[t] .. off[t + 1]) (offsets in hashes).  No hash: status[t] = 0 (the reference's null) and a zero root; one
   hash: itself; otherwise pairs level by level, an odd last node paired with itself.  The device forms also take
   n_hashes >= off[n_trees], which sizes the context's workspace. */
int lcb_merkle_root_batch(uint8_t *roots_out, uint8_t *status, const uint8_t *hashes, const uint64_t *off, size_t n_trees);
int lcb_ctx_merkle_root_dev(lcb_ctx *ctx, uint8_t *roots_out, uint8_t *status, const uint8_t *hashes, const uint64_t *off,
                            size_t n_trees, size_t n_hashes, void *stream);
int lcb_merkle_root_dev(uint8_t *roots_out, uint8_t *status, const uint8_t *hashes, const uint64_t *off, size_t n_trees,
                        size_t n_hashes, void *stream);

/* ------------------------------------------------------------------ secp256k1 ECDSA header signatures
   RootProtocol checks every SignedHeaderMessage with
     DefaultCrypto.VerifySignatureHashed(header.Keccak(), signature, EcdsaPublicKeySet[idx].EncodeCompressed(),
                                         useNewChainId)            (RootProtocol.cs:91-105, DefaultCrypto.cs:79-101)
   accept[i] = 1 exactly when the reference returns true: signature i is sig_len bytes (must equal 65 for the old
   chain id, 66 for the new one, DefaultCrypto.cs:26-29), its recovery id (sig[64], or sig[64] * 256 + sig[65]) gives
   (enc - 36) / 2 / chain_id in [0, 3] (C# int arithmetic; chain_id 0 rejects everything), r || s (big-endian) parse
   below n, s <= (n - 1) / 2, and x(u1 G + u2 Q) mod n == r with u1 = z / s, u2 = r / s, z = hash mod n (libsecp256k1
   semantics; Secp256k1.Net 0.1.55 / Secp256k1.Native 0.1.20, Lachain.Crypto.csproj:21-22).  key_idx[i] selects the
   key; an index out of range or a key that fails secp256k1_ec_pubkey_parse (33-byte 02/03 or 65-byte 04/06/07
   encodings) rejects.  `chain_id` is TransactionUtils.ChainId(use_new_chain_id) (TransactionUtils.cs:25-28).
   A key set keeps the validators' keys resident on the device with a 270 KB fixed-base table per key, built once;
   the host-pointer calls cache the last key list they saw in the calling thread's context. */
typedef struct lcb_ecdsa_keyset lcb_ecdsa_keyset;
/* BlockHeader (block.proto:7-15) as raw bytes; hashed as HashUtils.Keccak(BlockHeader) (HashUtils.cs:40-53) */
typedef struct {
    uint64_t index;
    uint8_t prev_block_hash[32];
    uint8_t merkle_root[32];
    uint8_t state_hash[32];
    uint64_t nonce;
} lcb_block_header;
lcb_ecdsa_keyset *lcb_ecdsa_keyset_create(const uint8_t *pubkeys, size_t pk_len, size_t n_keys);
void lcb_ecdsa_keyset_destroy(lcb_ecdsa_keyset *ks);
size_t lcb_ecdsa_keyset_size(const lcb_ecdsa_keyset *ks);
int lcb_ecdsa_keyset_valid(const lcb_ecdsa_keyset *ks, uint8_t *ok_out);   /* per key: parsed (1) or not (0) */
/* host pointers; hashes: n x 32 bytes (the reference's messageHash) */
int lcb_ecdsa_verify_hashed_batch(uint8_t *accept, const uint8_t *hashes, const uint8_t *sigs, size_t sig_len,
                                  const uint8_t *pubkeys, size_t pk_len, size_t n_keys, const int32_t *key_idx,
                                  size_t n, int use_new_chain_id, int32_t chain_id);
/* RootProtocol's whole check: header.Index == era (RootProtocol.cs:94-96), Keccak of the header, then the above */
int lcb_root_header_verify_batch(uint8_t *accept, const lcb_block_header *headers, uint64_t era, const uint8_t *sigs,
                                 size_t sig_len, const uint8_t *pubkeys, size_t pk_len, size_t n_keys,
                                 const int32_t *key_idx, size_t n, int use_new_chain_id, int32_t chain_id);
int lcb_header_keccak_batch(uint8_t *hashes, const lcb_block_header *headers, size_t n);
/* device pointers, enqueued on `stream` in a context (NULL = the calling thread's default context) */
int lcb_ctx_ecdsa_verify_hashed_dev(lcb_ctx *ctx, uint8_t *accept, const uint8_t *hashes, const uint8_t *sigs,
                                    size_t sig_len, const int32_t *key_idx, size_t n, const lcb_ecdsa_keyset *ks,
                                    int use_new_chain_id, int32_t chain_id, void *stream);
int lcb_ctx_root_header_verify_dev(lcb_ctx *ctx, uint8_t *accept, const uint8_t *headers, uint64_t era,
                                   const uint8_t *sigs, size_t sig_len, const int32_t *key_idx, size_t n,
                                   const lcb_ecdsa_keyset *ks, int use_new_chain_id, int32_t chain_id, void *stream);
/* signing side (EcdsaKeyPair / DefaultCrypto.SignHashed, DefaultCrypto.cs:107-137) with caller-given nonces (not
   RFC 6979, so signature bytes differ from libsecp256k1's for the same key and hash; every one verifies): key
   derivation out33 = compressed d G, and r || s (low s) || v encoded as SignHashed encodes it.  ok[i] = 0 for a
   private key or nonce outside [1, n) or a zero r / s.  Used for synthetic inputs and the node's own header. */
int lcb_ecdsa_pubkey_batch(uint8_t *out33, uint8_t *ok, const uint8_t *privs, size_t n);
int lcb_ecdsa_sign_hashed_batch(uint8_t *sigs_out, uint8_t *ok, const uint8_t *hashes, const uint8_t *privs,
                                const uint8_t *nonces, size_t n, int use_new_chain_id, int32_t chain_id);
int lcb_ctx_ecdsa_pubkey_dev(lcb_ctx *ctx, uint8_t *out33, uint8_t *ok, const uint8_t *privs, size_t n, void *stream);
int lcb_ctx_ecdsa_sign_hashed_dev(lcb_ctx *ctx, uint8_t *sigs_out, uint8_t *ok, const uint8_t *hashes,
                                  const uint8_t *privs, const uint8_t *nonces, size_t n, int use_new_chain_id,
                                  int32_t chain_id, void *stream);
int lcb_ecdsa_pubkey_dev(uint8_t *out33, uint8_t *ok, const uint8_t *privs, size_t n, void *stream);
int lcb_ecdsa_sign_hashed_dev(uint8_t *sigs_out, uint8_t *ok, const uint8_t *hashes, const uint8_t *privs,
                              const uint8_t *nonces, size_t n, int use_new_chain_id, int32_t chain_id, void *stream);
/* kernel milliseconds of the last verification in the context: header hash (0 if hashes were given), scalars, verify */
int lcb_ctx_ecdsa_phase_ms(lcb_ctx *ctx, float ms[3]);
int lcb_ecdsa_phase_ms(float ms[3]);
int lcb_ecdsa_verify_hashed_dev(uint8_t *accept, const uint8_t *hashes, const uint8_t *sigs, size_t sig_len,
                                const int32_t *key_idx, size_t n, const lcb_ecdsa_keyset *ks, int use_new_chain_id,
                                int32_t chain_id, void *stream);
int lcb_root_header_verify_dev(uint8_t *accept, const uint8_t *headers, uint64_t era, const uint8_t *sigs,
                               size_t sig_len, const int32_t *key_idx, size_t n, const lcb_ecdsa_keyset *ks,
                               int use_new_chain_id, int32_t chain_id, void *stream);

/* ------------------------------------------------------------------ secp256k1 public-key recovery (transaction senders)
   The reference authenticates every transaction by recovery: TransactionVerifier.VerifyTransactions
   (TransactionVerifier.cs:72-91) queues a block's receipts and its worker runs, per receipt,
     receipt.RecoverPublicKey -> DefaultCrypto.RecoverSignatureHashed -> ComputeAddress -> compare with Transaction.From
   (TransactionVerifier.cs:124-130; CryptoUtils.cs:53-58; DefaultCrypto.cs:146-168,197-200); the VM's ecrecover handlers
   (ExternalHandler.cs:1197,1225,1242) call the same and SpecialRecoverSignatureHashed (DefaultCrypto.cs:170-195).
   Per item: 32-byte hash, signature r || s || v at stride sig_len.  An item recovers when sig_len is 65 (old chain id)
   or 66 (new) as use_new_chain_id says, recId = (v - 36) / 2 / chain_id (truncating; chain id 0 fails) lies in [0, 3],
   r and s lie in [1, n), r + n < p when recId & 2, x(R) is on the curve and Q = r^-1 (s R - z G) is not infinity
   (libsecp256k1's secp256k1_ecdsa_recover; there is NO low-s rule on recovery).  Where the reference throws, ok[i] = 0
   and the item's output bytes are zero; nothing fails the call.  pub33_out (33 B compressed key per item) and
   addr20_out (Keccak-256(x || y)[12:], 20 B per item) may each be null. */
int lcb_ecdsa_recover_hashed_batch(uint8_t *pub33_out, uint8_t *addr20_out, uint8_t *ok, const uint8_t *hashes,
                                   const uint8_t *sigs, size_t sig_len, size_t n, int use_new_chain_id,
                                   int32_t chain_id);
/* SpecialRecoverSignatureHashed: 65-byte signatures with v = 27 (recId 0) or 28 (recId 1), no chain id */
int lcb_ecdsa_special_recover_hashed_batch(uint8_t *pub33_out, uint8_t *addr20_out, uint8_t *ok, const uint8_t *hashes,
                                           const uint8_t *sigs, size_t sig_len, size_t n);
/* The cache-miss branch of TransactionVerifier.VerifyTransactionImmediately (TransactionVerifier.cs:124-130):
   accept[i] = the signature recovers and the recovered address equals from20[i], on hashes the caller already holds.
   lcb_receipts_verify_batch (below) is the whole method from the receipt's fields: it computes RawHash and FullHash on
   the device and includes the receipt.Hash == FullHash check (line 115).  The reference's cached-key branch is VerifySignatureHashed
   (lcb_ecdsa_verify_hashed_batch), which enforces low s; this branch does not, exactly as in the reference. */
int lcb_tx_verify_batch(uint8_t *accept, const uint8_t *hashes, const uint8_t *sigs, size_t sig_len,
                        const uint8_t *from20, size_t n, int use_new_chain_id, int32_t chain_id);
/* device-pointer forms on a stream (asynchronous), with and without an explicit context */
int lcb_ctx_ecdsa_recover_hashed_dev(lcb_ctx *ctx, uint8_t *pub33_out, uint8_t *addr20_out, uint8_t *ok,
                                     const uint8_t *hashes, const uint8_t *sigs, size_t sig_len, size_t n,
                                     int use_new_chain_id, int32_t chain_id, void *stream);
int lcb_ctx_ecdsa_special_recover_hashed_dev(lcb_ctx *ctx, uint8_t *pub33_out, uint8_t *addr20_out, uint8_t *ok,
                                             const uint8_t *hashes, const uint8_t *sigs, size_t sig_len, size_t n,
                                             void *stream);
int lcb_ctx_tx_verify_dev(lcb_ctx *ctx, uint8_t *accept, const uint8_t *hashes, const uint8_t *sigs, size_t sig_len,
                          const uint8_t *from20, size_t n, int use_new_chain_id, int32_t chain_id, void *stream);
int lcb_ecdsa_recover_hashed_dev(uint8_t *pub33_out, uint8_t *addr20_out, uint8_t *ok, const uint8_t *hashes,
                                 const uint8_t *sigs, size_t sig_len, size_t n, int use_new_chain_id, int32_t chain_id,
                                 void *stream);
int lcb_ecdsa_special_recover_hashed_dev(uint8_t *pub33_out, uint8_t *addr20_out, uint8_t *ok, const uint8_t *hashes,
                                         const uint8_t *sigs, size_t sig_len, size_t n, void *stream);
int lcb_tx_verify_dev(uint8_t *accept, const uint8_t *hashes, const uint8_t *sigs, size_t sig_len, const uint8_t *from20,
                      size_t n, int use_new_chain_id, int32_t chain_id, void *stream);
/* kernel milliseconds of the last recovery in the context: scalars, recovery, finish */
int lcb_ctx_ecdsa_recover_phase_ms(lcb_ctx *ctx, float ms[3]);
int lcb_ecdsa_recover_phase_ms(float ms[3]);
/* Keccak-256 (original 0x01 padding: KeccakBytes, the RawHash of a transaction's RLP for RecoverSignature,
   DefaultCrypto.cs:139-144) of n messages: message i is data[off[i] .. off[i + 1]); off has n + 1 entries */
int lcb_keccak256_batch(uint8_t *out32, const uint8_t *data, const uint64_t *off, size_t n);
int lcb_ctx_keccak256_dev(lcb_ctx *ctx, uint8_t *out32, const uint8_t *data, const uint64_t *off, size_t n, void *stream);
int lcb_keccak256_dev(uint8_t *out32, const uint8_t *data, const uint64_t *off, size_t n, void *stream);

/* ------------------------------------------------------------------ transaction hashing and receipt verification
   A receipt goes in as fields; its RLP is formed and hashed on the device (k_txhash.hip), exactly as
   TransactionUtils.GetEthTx / Rlp / RlpWithSignature / RawHash / FullHash produce it (TransactionUtils.cs:30-105,
   HexUtils.cs:88-92, Nethereum RLP.EncodeElement / EncodeList):
     RawHash  = Keccak-256(list[nonce, gasPrice, gasLimit, to, value, invocation, chainId, "", ""])
     FullHash = Keccak-256(list[nonce, gasPrice, gasLimit, to, value, invocation, v, r, s])
   nonce is the empty string when 0, otherwise minimal big-endian; gasPrice, gasLimit and chainId are minimal
   big-endian with zero as the one byte 00; to is its 20 bytes or the empty string; value is its 32 bytes with leading
   zero bytes stripped (nothing left for zero); r = sig[0:32] and s = sig[32:64] likewise; v = sig[64:sig_len] with
   leading zeros stripped unless it is all zero, when it stays whole (00, or 82 00 00 for two bytes).  These rules
   reproduce the five strings and four hashes of CryptographyTest.cs:208-274, the zero-signature encoding of system
   transactions among them.  A signature with only one of r, s zero is pinned by no reference vector; the same rule is
   applied to it (such a signature never recovers).
   Item i: txs[i], invocation bytes invocations[inv_off[i] .. inv_off[i + 1]) (inv_off has n + 1 entries), signature
   sigs + sig_len * i, claimed hash hashes32 + 32 * i.  sig_len must be 65 for the old chain id and 66 for the new one;
   `chain_id` is TransactionUtils.ChainId(use_new_chain_id).  A call fails (-1) for a missing pointer, a wrong sig_len, a
   negative chain id and, in the host-pointer forms, for decreasing offsets, an invocation of 2^31 bytes or more and a
   to_len other than 0 or 20; the device-pointer forms cannot read their inputs and trust the caller for these three
   (txs and inv_off 8-byte aligned).  A bad item never fails a call. */
typedef struct {
    uint64_t nonce, gas_price, gas_limit;
    uint8_t value[32];          /* UInt256 buffer, big-endian */
    uint8_t to[20];
    uint8_t from[20];           /* Transaction.From: read by the receipt calls only */
    uint32_t to_len;            /* 20, or 0 for an empty To */
    uint32_t reserved;          /* 0 */
} lcb_tx_fields;                /* 104 bytes */
/* raw32_out / full32_out: n x 32 bytes, each may be null; with sigs == NULL only raw32_out is written */
int lcb_tx_hash_batch(uint8_t *raw32_out, uint8_t *full32_out, const lcb_tx_fields *txs, const uint8_t *invocations,
                      const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len, size_t n, int use_new_chain_id,
                      int32_t chain_id);
int lcb_ctx_tx_hash_dev(lcb_ctx *ctx, uint8_t *raw32_out, uint8_t *full32_out, const lcb_tx_fields *txs,
                        const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len, size_t n,
                        int use_new_chain_id, int32_t chain_id, void *stream);
int lcb_tx_hash_dev(uint8_t *raw32_out, uint8_t *full32_out, const lcb_tx_fields *txs, const uint8_t *invocations,
                    const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len, size_t n, int use_new_chain_id,
                    int32_t chain_id, void *stream);
/* TransactionVerifier.VerifyTransactionImmediately(receipt, useNewChainId, cacheEnabled: false)
   (TransactionVerifier.cs:109-143) per item, in one call: hashing, the hash check, the recovery (the rules of
   lcb_ecdsa_recover_hashed_batch: no low-s rule) and the From comparison all run on the device and the raw hashes
   never leave it.  detail[i] bit 0: hashes32[i] == FullHash; bit 1: the signature recovers from RawHash; bit 2: the
   recovered address equals txs[i].from.  accept[i] = (detail[i] == 7); detail may be null.  Nothing throws. */
int lcb_receipts_verify_batch(uint8_t *accept, uint8_t *detail, const lcb_tx_fields *txs, const uint8_t *invocations,
                              const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len, const uint8_t *hashes32,
                              size_t n, int use_new_chain_id, int32_t chain_id);
int lcb_ctx_receipts_verify_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *detail, const lcb_tx_fields *txs,
                                const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len,
                                const uint8_t *hashes32, size_t n, int use_new_chain_id, int32_t chain_id, void *stream);
int lcb_receipts_verify_dev(uint8_t *accept, uint8_t *detail, const lcb_tx_fields *txs, const uint8_t *invocations,
                            const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len, const uint8_t *hashes32, size_t n,
                            int use_new_chain_id, int32_t chain_id, void *stream);
/* The same for the receipts of n_blocks blocks: block b holds receipts tx_off[b] .. tx_off[b + 1] (tx_off runs from 0 to
   n), and root_ok[b] = (MerkleTree.ComputeRoot(the given hashes of block b) ?? Zero) == expected_roots[b]
   (BlockManager.cs:690-694; lcb_merkle_root_batch's tree).  A block without transactions gives root_ok = (expected is
   all zero). */
int lcb_block_txs_verify_batch(uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs,
                               const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len,
                               const uint8_t *hashes32, size_t n, const uint64_t *tx_off, const uint8_t *expected_roots,
                               size_t n_blocks, int use_new_chain_id, int32_t chain_id);
int lcb_ctx_block_txs_verify_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs,
                                 const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len,
                                 const uint8_t *hashes32, size_t n, const uint64_t *tx_off, const uint8_t *expected_roots,
                                 size_t n_blocks, int use_new_chain_id, int32_t chain_id, void *stream);
int lcb_block_txs_verify_dev(uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs,
                             const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len,
                             const uint8_t *hashes32, size_t n, const uint64_t *tx_off, const uint8_t *expected_roots,
                             size_t n_blocks, int use_new_chain_id, int32_t chain_id, void *stream);
/* kernel milliseconds of the last transaction call enqueued in the context (the *_dev forms; NULL = the calling thread's
   default context): hashing, recovery with the decision, roots */
int lcb_ctx_tx_phase_ms(lcb_ctx *ctx, float ms[3]);
int lcb_tx_phase_ms(float ms[3]);

/* raw-transaction ingress: the other direction.  n signed wire transactions (RLP) go in; the decoded records,
   signatures, RawHash, FullHash, the sender and the pool's signature decision come out of one call
   (TransactionServiceWeb3.SendRawTransaction, TransactionServiceWeb3.cs:184-215, down to TransactionPool.Add's
   signature check, TransactionPool.cs:130-143).  The decode runs on the device (k_rawtx.hip) and treats every byte as
   hostile.  Item i is raw[raw_off[i] .. raw_off[i + 1]).  The signature width follows use_new_chain_id (66, else 65).
   The decoder is strict: status[i] names the first rule an item breaks, and such an item gets zero bytes in every other
   output; the caller sends it down its host path (what Nethereum's decoder makes of malformed or non-canonical RLP is
   pinned by no reference vector, and the refusals are a conservative superset of where the reference throws):
     NOT_LIST     an empty item, or a first byte below c0
     LIST_LENGTH  a long list header with more than 4 length bytes, running past the item, with a zero first length
                  byte or a length below 56; or header + payload != the item's length
     ELEMENT      among the nine elements: a list byte, a header or body running past the payload, 81 before a byte
                  below 80, a long form with more than 4 length bytes, a zero first length byte or a length below 56
     COUNT        fewer than nine elements, or bytes left after the ninth (a tenth is never parsed)
     WIDTH        nonce, gasPrice, gasLimit above 8 bytes; to neither 0 nor 20; value, r, s above 32; v not sig_len - 64
   Decoded integers are the big-endian value of their bytes (empty: 0); value, r, s are left-padded; sigs_out[i] =
   r || s || v; inv_span_out[2 i], [2 i + 1] = the invocation's offset in raw and its length (it is not copied).
   detail[i]: SAME_ENCODING = elements 0-5 as they stand on the wire are Lachain's own encoding of the decoded fields
   (TransactionUtils.cs:30-48: no leading zero byte in nonce or value, gasPrice / gasLimit not empty and without a
   leading zero unless the lone byte 00); CHAIN_OK = v is 2 chain_id + 35 or + 36 (:203); RECOVERS = the signature
   recovers from RawHash (lcb_ecdsa_recover_hashed_batch's rules, no low-s rule).  raw32_out / full32_out: RawHash under
   chain_id and FullHash of the decoded fields (what SendRawTransaction returns).  accept[i] = status 0 and detail 7;
   txs_out[i].from is the recovered address where accept[i] is 1, zero otherwise.  status is required, every other
   output may be null; with accept == NULL the recovery is skipped and detail carries bits 0 and 1 only.
   A call fails (-1) for a missing status, raw or raw_off, chain_id <= 0, a chain id whose 2 chain_id + 36 does not fit
   sig_len - 64 bytes (above 109 old, 32749 new) and, in the host-pointer form, for decreasing offsets or an item of 2^31
   bytes or more; the device forms trust the caller for the offsets (raw_off, txs_out and inv_span_out 8-byte aligned)
   and trust nothing inside the items.  A bad item never fails a call. */
#define LCB_RAWTX_OK          0
#define LCB_RAWTX_NOT_LIST    1
#define LCB_RAWTX_LIST_LENGTH 2
#define LCB_RAWTX_ELEMENT     3
#define LCB_RAWTX_COUNT       4
#define LCB_RAWTX_WIDTH       5
#define LCB_RAWTX_SAME_ENCODING 1
#define LCB_RAWTX_CHAIN_OK      2
#define LCB_RAWTX_RECOVERS      4
int lcb_raw_txs_ingest_batch(uint8_t *accept, uint8_t *status, uint8_t *detail, lcb_tx_fields *txs_out,
                             uint64_t *inv_span_out, uint8_t *sigs_out, uint8_t *raw32_out, uint8_t *full32_out,
                             const uint8_t *raw, const uint64_t *raw_off, size_t n, int use_new_chain_id, int32_t chain_id);
int lcb_ctx_raw_txs_ingest_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *status, uint8_t *detail, lcb_tx_fields *txs_out,
                               uint64_t *inv_span_out, uint8_t *sigs_out, uint8_t *raw32_out, uint8_t *full32_out,
                               const uint8_t *raw, const uint64_t *raw_off, size_t n, int use_new_chain_id,
                               int32_t chain_id, void *stream);
int lcb_raw_txs_ingest_dev(uint8_t *accept, uint8_t *status, uint8_t *detail, lcb_tx_fields *txs_out,
                           uint64_t *inv_span_out, uint8_t *sigs_out, uint8_t *raw32_out, uint8_t *full32_out,
                           const uint8_t *raw, const uint64_t *raw_off, size_t n, int use_new_chain_id, int32_t chain_id,
                           void *stream);
/* kernel milliseconds of the context's last ingress: decode and hashing, recovery, finish */
int lcb_ctx_rawtx_phase_ms(lcb_ctx *ctx, float ms[3]);
int lcb_rawtx_phase_ms(float ms[3]);

/* ------------------------------------------------------------------ state trie: node hashes, checks, roots
   Block.Header.StateHash is the Keccak-256 of six trie roots (BlockchainSnapshot.cs:71-80); each root is the hash of a
   32-way hash-array-mapped trie (Lachain.Storage/Trie/TrieHashMap.cs, LeafNode.cs, InternalNode.cs):
     leaf     = Keccak-256(int32 LE KeyHash.Length || KeyHash || Value)
     internal = Keccak-256(label_0 || child_0 || label_1 || child_1 ...), labels = the set bits of ChildrenMask in
                ascending order, zipped with the child hashes: pairs as far as both last (IsConsistent hashes a node with
                too few or too many child hashes the same way)
   Kernels: k_trie.hip.  No reference vector pins a trie hash; these entry points are pinned by the literal restatement
   tests/pyref/trie.py over a Keccak that the reference's vector pins.  Storage itself (RocksDB, node ids and versions,
   caches) stays with the caller: only node and state hashing is provided.
   Items are given as in lcb_keccak256_batch: item i is the bytes [off[i], off[i + 1]) of its array.  The host-pointer
   forms check what they can read; the device-pointer forms trust the caller for the records and offsets (nodes 4-byte,
   offset / reference / order arrays 8-byte aligned). */
typedef struct {
    uint32_t kind;              /* 0 leaf, 1 internal (NodeType's values) */
    uint32_t mask;              /* internal: ChildrenMask */
    uint32_t key_len;           /* leaf: KeyHash.Length; any value is legal, as in the reference */
    uint32_t reserved;          /* 0 */
} lcb_trie_node;                /* 16 bytes */
/* (a) NodeStorage.IsConsistent, TrieHashMap.RecalculateHash / CheckAllNodeHashes, the LeafNode constructor and
   InternalNode.UpdateHash for a batch.  A leaf's bytes are KeyHash || Value; an internal node's bytes are its child hashes,
   32 bytes each, in label order.  out32[i] = the node's hash; accept[i] = (hash == expected32[i]).  out32, or expected32
   and accept, may be null.  The host form fails (-1) for a kind above 1, a non-zero reserved, internal bytes that are no
   multiple of 32 and a key_len beyond the item. */
int lcb_trie_node_hash_batch(uint8_t *out32, uint8_t *accept, const lcb_trie_node *nodes, const uint8_t *data,
                             const uint64_t *data_off, const uint8_t *expected32, size_t n);
int lcb_ctx_trie_node_hash_dev(lcb_ctx *ctx, uint8_t *out32, uint8_t *accept, const lcb_trie_node *nodes,
                               const uint8_t *data, const uint64_t *data_off, const uint8_t *expected32, size_t n,
                               void *stream);
int lcb_trie_node_hash_dev(uint8_t *out32, uint8_t *accept, const lcb_trie_node *nodes, const uint8_t *data,
                           const uint64_t *data_off, const uint8_t *expected32, size_t n, void *stream);
/* (b) TrieHashMap.InsertAllNodes, and the commit of a block's updates when hashing is deferred: every node of the batch
   is hashed once, children before parents.  Leaf i has bytes data[data_off[i] .. data_off[i + 1]) and no children.
   Internal node i has children child_ref[child_off[i] .. child_off[i + 1]) in label order, popcount(mask) of them: ref >= 0
   is node ref of this batch (any array order; a child may have several parents), ref < 0 is literals32[~ref], the hash of
   a clean subtree outside the batch.  hash_out32: n x 32 bytes.  The host form computes each node's height and launches
   one pass per height; it fails (-1) for a reference out of range, a cycle and a child count other than popcount(mask).
   The device forms take the level order from the caller: order (device, n node indices, level 0 first) and level_off
   (HOST memory, n_levels + 1 entries into order); level l may reference nodes of lower levels only. */
int lcb_trie_rehash_batch(uint8_t *hash_out32, const lcb_trie_node *nodes, const uint8_t *data, const uint64_t *data_off,
                          const uint64_t *child_off, const int64_t *child_ref, const uint8_t *literals32, size_t n_literals,
                          size_t n);
int lcb_ctx_trie_rehash_dev(lcb_ctx *ctx, uint8_t *hash_out32, const lcb_trie_node *nodes, const uint8_t *data,
                            const uint64_t *data_off, const uint64_t *child_off, const int64_t *child_ref,
                            const uint8_t *literals32, const uint64_t *order, const uint64_t *level_off, size_t n_levels,
                            size_t n, void *stream);
int lcb_trie_rehash_dev(uint8_t *hash_out32, const lcb_trie_node *nodes, const uint8_t *data, const uint64_t *data_off,
                        const uint64_t *child_off, const int64_t *child_ref, const uint8_t *literals32,
                        const uint64_t *order, const uint64_t *level_off, size_t n_levels, size_t n, void *stream);
/* (c) The root hashes of B tries given as key/value sets: trie b holds items trie_off[b] .. trie_off[b + 1] (trie_off runs
   from 0 to the item count).  keys_hashed = 0: the key hash is the Keccak-256 of the key, computed on the device
   (TrieHashMap.Hash); 1: the keys are 32-byte key hashes.  The trie the reference's folding rules keep (ModifyInternalNode,
   SplitLeafNode) is canonical — a subtree with one key is that leaf, a prefix shared by two or more key hashes is an
   internal node, single-child chain nodes included — so the root depends on the set alone and is built here by sorting.
   roots32[b] = the root, status[b] = 1; an empty set gives the zero hash (GetHash's fallback) with status 1; a set on which
   the reference throws (two equal key hashes; two key hashes that differ in bit 255 only) gives status 0 and a zero root,
   and the other tries of the call are unaffected.  The construction runs on the device; the call reads one word (the
   longest common prefix) back and therefore synchronises the stream once, the device forms included.  The built nodes
   are not returned. */
int lcb_trie_root_batch(uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off,
                        const uint8_t *values, const uint64_t *val_off, const uint64_t *trie_off, size_t B, int keys_hashed);
int lcb_ctx_trie_root_dev(lcb_ctx *ctx, uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off,
                          const uint8_t *values, const uint64_t *val_off, const uint64_t *trie_off, size_t B, size_t n_items,
                          int keys_hashed, void *stream);
int lcb_trie_root_dev(uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off, const uint8_t *values,
                      const uint64_t *val_off, const uint64_t *trie_off, size_t B, size_t n_items, int keys_hashed,
                      void *stream);

/* ------------------------------------------------------------------ secp256k1 ECIES (the trustless DKG's envelopes)
   Every secret of the trustless key generation travels in DefaultCrypto.Secp256K1Encrypt and is opened by
   Secp256K1Decrypt (DefaultCrypto.cs:301-336): StartKeygen wraps one row per validator, HandleCommit opens a row and
   wraps N values, HandleSendValue opens a value (TrustlessKeygen.cs:63-76,90-109,111-135).  An envelope is
     eph_pub33 || nonce16 || C || tag16,   key = Secp256K1.Ecdh = SHA-256(compressed d P)
   (libsecp256k1's secp256k1_ecdh with its default hash), AES-256-GCM as BouncyCastle's GcmBlockCipher(AesEngine) with
   a 16-byte nonce, no associated data and a 16-byte tag (AesGcmEncrypt / AesGcmDecrypt, DefaultCrypto.cs:267-299; the
   nonce is not 96 bits, so J0 = GHASH(nonce || 0^64 || [128]_64), NIST SP 800-38D).  Kernels: k_ecies.hip.
   Items are given as in lcb_keccak256_batch: item i is the bytes [off[i], off[i + 1]) of its array, off has n + 1
   non-decreasing entries.  Where the reference throws — a malformed or off-curve key (the 33-byte slot takes the
   prefixes 0x02 and 0x03 only), a scalar outside [1, n), an envelope shorter than 65 bytes or a GCM item shorter than
   32, a tag mismatch — the item gets ok[i] = 0 and zero output bytes and its neighbours are unaffected; only bad
   arguments (a null pointer, a decreasing offset) fail the call.  n = 0 is a successful no-op.
   The ephemeral private keys and the nonces come from the caller, as the signing entry points take their nonces: the
   caller MUST draw both from a cryptographically secure generator and use each once.  A repeated (key, nonce) pair
   gives away the GCM authentication key and the xor of the plaintexts.
   No constant-time claim is made on the GPU (table lookups and skipped zero digits depend on the scalar): the
   standing of lcb_ecdsa_sign_hashed_batch, lcb_ts_sign and lcb_tpke_partial_decrypt.  Workspaces and staging copies
   that held private, ephemeral or session keys are cleared on the stream before a call returns. */
/* key32_out[i] = SHA-256 of the compressed d P (Secp256K1.Ecdh); ok[i] = 0 and zero bytes where libsecp256k1 returns
   0.  Item i uses scalars32[scalar_idx[i]] (an index >= n_scalars fails the item), or scalars32[i] when scalar_idx is
   null (n_scalars is then ignored) */
int lcb_secp_ecdh_batch(uint8_t *key32_out, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
                        const uint32_t *scalar_idx, size_t n_scalars, size_t n);
/* AesGcmEncrypt with caller-given nonces: out item i = nonce || C || tag at out + (pt_off[i] - pt_off[0]) + 32 i */
int lcb_aes256_gcm_encrypt_batch(uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16, const uint8_t *pt,
                                 const uint64_t *pt_off, size_t n);
/* AesGcmDecrypt: the plaintexts are packed in item order, item i after the plaintexts of the items before it (a
   rejected item of valid length keeps its zeroed slot, an item shorter than 32 bytes takes none): at ct_off[i] -
   ct_off[0] - 32 i when no item is too short.  pt_out holds at most ct_off[n] - ct_off[0] bytes */
int lcb_aes256_gcm_decrypt_batch(uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                                 const uint64_t *ct_off, size_t n);
/* Secp256K1Encrypt: out item i = eph_pub33 || nonce || C || tag, 65 bytes longer than its plaintext, at
   out + (pt_off[i] - pt_off[0]) + 65 i; the ephemeral public key is eph_priv32[i] G */
int lcb_secp256k1_encrypt_batch(uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33, const uint8_t *eph_priv32,
                                const uint8_t *nonces16, const uint8_t *pt, const uint64_t *pt_off, size_t n);
/* Secp256K1Decrypt: item i is opened with privs32[priv_idx[i]], or privs32[i] when priv_idx is null; the plaintexts
   are packed as by lcb_aes256_gcm_decrypt_batch with 65 bytes of overhead per item */
int lcb_secp256k1_decrypt_batch(uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32, const uint32_t *priv_idx,
                                size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n);
/* device-pointer forms on a stream (asynchronous), with and without an explicit context.  They trust the offsets
   (which are absolute into pt / ct; the output positions are as above) */
int lcb_ctx_secp_ecdh_dev(lcb_ctx *ctx, uint8_t *key32_out, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
                          const uint32_t *scalar_idx, size_t n_scalars, size_t n, void *stream);
int lcb_ctx_aes256_gcm_encrypt_dev(lcb_ctx *ctx, uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16,
                                   const uint8_t *pt, const uint64_t *pt_off, size_t n, void *stream);
int lcb_ctx_aes256_gcm_decrypt_dev(lcb_ctx *ctx, uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                                   const uint64_t *ct_off, size_t n, void *stream);
int lcb_ctx_secp256k1_encrypt_dev(lcb_ctx *ctx, uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33,
                                  const uint8_t *eph_priv32, const uint8_t *nonces16, const uint8_t *pt,
                                  const uint64_t *pt_off, size_t n, void *stream);
int lcb_ctx_secp256k1_decrypt_dev(lcb_ctx *ctx, uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32,
                                  const uint32_t *priv_idx, size_t n_privs, const uint8_t *ct, const uint64_t *ct_off,
                                  size_t n, void *stream);
int lcb_secp_ecdh_dev(uint8_t *key32_out, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
                      const uint32_t *scalar_idx, size_t n_scalars, size_t n, void *stream);
int lcb_aes256_gcm_encrypt_dev(uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16, const uint8_t *pt,
                               const uint64_t *pt_off, size_t n, void *stream);
int lcb_aes256_gcm_decrypt_dev(uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                               const uint64_t *ct_off, size_t n, void *stream);
int lcb_secp256k1_encrypt_dev(uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33, const uint8_t *eph_priv32,
                              const uint8_t *nonces16, const uint8_t *pt, const uint64_t *pt_off, size_t n, void *stream);
int lcb_secp256k1_decrypt_dev(uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32, const uint32_t *priv_idx,
                              size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n, void *stream);
/* kernel milliseconds of the last ECIES call in the context: scalars, multiplication, finish, GCM (with the
   ephemeral public keys of an encryption); a phase the call did not run reads 0 */
int lcb_ctx_ecies_phase_ms(lcb_ctx *ctx, float ms[4]);
int lcb_ecies_phase_ms(float ms[4]);

/* ------------------------------------------------------------------ aggregation queue (one share per call)
   The consensus code verifies one share per call from many protocol threads (HoneyBadger.cs:156-158,211-212,
   ThresholdSigner.cs:62, AbstractProtocol.cs:46-47).  A queue aggregates such calls into GPU batches: submit
   returns a ticket (> 0, or -1 on bad arguments), a worker thread runs the pending shares as one batch when
   max_batch are pending or the oldest has waited max_delay_us, and lcb_queue_wait returns the share's decision
   (1 accept, 0 reject, -1 batch error / unknown or already-waited ticket).  Decisions equal the batch entry
   points' (PublicKey.VerifyShare, TPKE/PublicKey.cs:88-92; ValidateSignature, ThresholdSignature/PublicKey.cs:16-21).
   destroy flushes and runs everything still pending; stats: {batches, shares, largest batch}. */
typedef struct lcb_queue lcb_queue;
lcb_queue *lcb_queue_create(size_t max_batch, uint32_t max_delay_us);
void lcb_queue_destroy(lcb_queue *q);
int64_t lcb_queue_tpke_verify(lcb_queue *q, const uint8_t y48[48], const uint8_t u48[48], const uint8_t *v,
                              size_t v_len, const uint8_t w96[96], const uint8_t ui48[48]);
int64_t lcb_queue_ts_verify(lcb_queue *q, const uint8_t pk48[48], const uint8_t *msg, size_t msg_len,
                            const uint8_t sig96[96]);
/* prepare a TPKE ciphertext (U || V || W: hash-to-G2 of U || V and both line sets) on the worker its shares go to,
   ahead of them — the reference decrypts every ciphertext of the common subset (HoneyBadger.cs:144-146) before it
   handles the other validators' shares for it (HoneyBadger.cs:190-213).  Asynchronous; 0 or -1 (bad arguments). */
int lcb_queue_tpke_prepare(lcb_queue *q, const uint8_t u48[48], const uint8_t *v, size_t v_len, const uint8_t w96[96]);
int lcb_queue_wait(lcb_queue *q, int64_t ticket);
int lcb_queue_flush(lcb_queue *q);
int lcb_queue_stats(lcb_queue *q, uint64_t out[3]);
const char *lcb_queue_last_error(lcb_queue *q);
/* flushes of at least min_shares shares use the randomized batch checks (lcb_tpke_verify_shares_batched /
   lcb_ts_verify_shares_batched, shares reordered by ciphertext / message inside the flush); 0 = exact checks only
   (the default) */
int lcb_queue_set_batched(lcb_queue *q, size_t min_shares);

/* ------------------------------------------------------------------ CommonCoin consumers (row a13)
   The combined signature's serialized bytes feed two consensus decisions:
   CoinResult.Parity = popcount(XOR of all bytes) is odd   (src/Lachain.Consensus/CommonCoin/CoinResult.cs:16-20)
   block nonce = little-endian u64 of the 8-byte XOR fold   (src/Lachain.Consensus/RootProtocol/RootProtocol.cs:316-322)
   Host forms take any byte length; the device form folds n 96-byte signatures (8-byte aligned) in one launch,
   either output nullable. */
int lcb_coin_parity(const uint8_t *sig_bytes, size_t len);
uint64_t lcb_coin_nonce(const uint8_t *sig_bytes, size_t len);
int lcb_coin_fold_dev(uint8_t *parity, uint64_t *nonce, const uint8_t *sigs96, size_t n, void *stream);

/* PrivateKeyShare.HashAndSign for a batch of (key, message) pairs (ThresholdSignature/PrivateKeyShare.cs:21-27) */
int lcb_ts_sign(uint8_t *sigs_out, const uint8_t *sks, const uint8_t *msg_data, const uint32_t *msg_off,
                const uint32_t *msg_idx, size_t n);

/* Batched Lagrange interpolation at 0 (MclBls12381.LagrangeInterpolate; PublicKeySet.AssembleSignature,
   ThresholdSignature/PublicKeySet.cs:34-42, and TPKE FullDecrypt, TPKE/PublicKey.cs:74-84).
   Problem j uses k = off[j+1]-off[j] entries starting at off[j]: x values as 32-byte Fr, y values serialized.
   status[j] = 1 ok, 0 on k == 0, zero x or duplicate x (mcl returns -1). */
int lcb_g1_lagrange_batch(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                          const uint32_t *off, size_t n_problems);
int lcb_g2_lagrange_batch(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                          const uint32_t *off, size_t n_problems);

/* Device-pointer forms of the batched Lagrange interpolation above (n_entries = off[n_problems]). */
int lcb_g1_lagrange_dev(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys, const uint32_t *off,
                        size_t n_problems, size_t n_entries, void *stream);
int lcb_g2_lagrange_dev(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys, const uint32_t *off,
                        size_t n_problems, size_t n_entries, void *stream);

/* G1 multi-scalar multiplication sum_i s_i P_i (serialized points, 32-byte LE scalars < r): the large-k form of
   MclBls12381.LagrangeInterpolate / mclBnG1_mulVec (TPKE/PublicKey.cs:83, ThresholdSignature/PublicKeySet.cs:31).
   Pippenger bucket method on the GPU (k_msm.hip).  Returns -1 on a malformed point or a scalar >= r. */
int lcb_g1_msm(uint8_t out[48], const uint8_t *points, const uint8_t *scalars, size_t n);

/* Device-resident MSM (BASELINE configs[3]).  points_aff: n x 96 B affine points in mcl's in-memory Fp layout
   (x then y, Montgomery form, 6 x u64 LE each = the x,y words of a normalized mclBnG1; (0,0) = infinity);
   scalars: n x 32 B LE, reduced mod r on the device.  out_jac: 144 B Jacobian result (mclBnG1 layout) in device
   memory.  window_bits = 0 picks the Pippenger window width from n (lcb_g1_msm_window).  Enqueued on `stream`
   (a hipStream_t); nothing is synchronised. */
int lcb_g1_msm_dev(void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n, int window_bits,
                   void *stream);
int lcb_g1_msm_window(size_t n);
/* GLV form of the same MSM for points of order r (e.g. generated as a_i G, or checked with a subgroup test):
   s_i = s1 + s2 lambda (lambda = z^2 - 1, s1 < 2^129, s2 < 2^128) over the 2n points P_i, phi(P_i) = (beta x, y):
   half the windows, so half the serial window combination and bucket reduction.  For a point with a component
   outside the r-subgroup phi(P) != lambda P and the result differs from lcb_g1_msm_dev's (which is exact for any
   point), so wire-supplied points (e.g. LagrangeInterpolate over shares) must use lcb_g1_msm_dev. */
int lcb_g1_msm_glv_dev(void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n, int window_bits,
                       void *stream);
int lcb_ctx_g1_msm_glv_dev(lcb_ctx *ctx, void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n,
                           int window_bits, void *stream);
int lcb_g1_msm_glv_window(size_t n);
/* per-phase device time (ms) of the last MSM: digits, sort, bucket bounds, bucket accumulation, bucket
   reduction, window combination (waits for the last MSM to finish) */
int lcb_g1_msm_phase_ms(float *ms, int n_phases);
/* 48-byte serialized G1 -> 96-byte affine device layout above; ok[i] = 0 for a malformed encoding (nullable) */
int lcb_g1_to_affine_dev(void *out_aff, uint8_t *ok, const uint8_t *points, size_t n, void *stream);
/* sum of k Jacobian G1 points (device, 144 B each, e.g. the per-GPU MSM partials after an RCCL all-gather);
   writes the serialized sum to out48 and/or the Jacobian sum to out_jac (device pointers, either nullable) */
int lcb_g1_jac_sum_dev(uint8_t *out48, void *out_jac, const void *parts, size_t k, void *stream);
int lcb_ctx_g1_jac_sum_dev(lcb_ctx *ctx, uint8_t *out48, void *out_jac, const void *parts, size_t k, void *stream);

/* batched scalar multiplication of the G1 / G2 generator or of given points (key generation, synthetic inputs) */
int lcb_g1_mul_batch(uint8_t *out, const uint8_t *points, int points_is_generator, const uint8_t *scalars, size_t n);
int lcb_g2_mul_batch(uint8_t *out, const uint8_t *points, int points_is_generator, const uint8_t *scalars, size_t n);
int lcb_g2_hash_batch(uint8_t *out, const uint8_t *msg_data, const uint32_t *msg_off, size_t n);

/* TPKE Utils.XorWithHash (BouncyCastle DigestRandomGenerator(Sha3Digest) keystream, TPKE/Utils.cs:12-19):
   host-side byte work, provided so a non-.NET host can finish FullDecrypt/Encrypt. */
void lcb_xor_with_hash(uint8_t *out, const uint8_t g1[48], const uint8_t *data, size_t len);

/* ------------------------------------------------------------------ TPKE keystream on the device (k_kdf.hip)
   Utils.XorWithHash for batches, and with it PublicKey.Encrypt and PublicKey.FullDecrypt in one call each: the
   keystream runs between (Encrypt) or behind (FullDecrypt) the kernels of lcb_tpke_encrypt_phase1 / _phase2 and
   lcb_tpke_combine_dev on one stream, and T = rY and u = sum lambda_i U_i never leave the device.  One item per lane:
   the generator's chain is sequential within an item (one Keccak permutation per 32 bytes), so these calls are for
   batches; a single item is faster through lcb_xor_with_hash.
   Items are packed as in the TPKE calls' v_data / v_off: item i is the bytes [off[i], off[i + 1]) of its array, with
   n + 1 non-decreasing uint32 offsets; every output is packed as its input, i.e. out item i lies at out + data_off[i].
   Items may start at any byte alignment.  out == data (in place) is allowed; any other overlap of an output with an
   input is not supported.  The *_dev forms take device pointers, are asynchronous on `stream`, trust their offsets and
   synchronise nothing; the host-pointer forms fail the call on a decreasing offset pair.  n = 0 is a successful no-op.
   T, u and r open the ciphertext: the device buffers of T and u and a host form's staged copy of r are cleared on the
   stream before the call returns.  No constant-time claim is made (the standing of the ECIES calls above). */
/* out item i = data item i ^ DigestRandomGenerator(Sha3Digest) seeded with seeds[seed_off[i] .. seed_off[i + 1]); a seed
   of any length, zero included (TPKE/Utils.cs:12-19 with a 48-byte G1 seed) */
int lcb_xor_with_hash_batch(uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off, const uint8_t *data,
                            const uint32_t *data_off, size_t n);
int lcb_ctx_xor_with_hash_dev(lcb_ctx *ctx, uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off,
                              const uint8_t *data, const uint32_t *data_off, size_t n, void *stream);
int lcb_xor_with_hash_dev(uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off, const uint8_t *data,
                          const uint32_t *data_off, size_t n, void *stream);
/* PublicKey.Encrypt for a batch with caller-supplied randomness r (TPKE/PublicKey.cs:25-37): U = rG (48 B per item),
   V = data ^ KDF(rY) (packed as data), W = r H(U || V) (96 B per item).  The host form fails where the two phases fail:
   "invalid public key or scalar" (y malformed, r >= the group order), "hash-to-G2 failed".  The *_dev form reports
   those per item: ok[i] = 0 (nullable), V item i zero bytes when the key or scalar is invalid. */
int lcb_tpke_encrypt_batch(uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, const uint8_t y[48], const uint8_t *r,
                           const uint8_t *data, const uint32_t *data_off, size_t n);
int lcb_ctx_tpke_encrypt_dev(lcb_ctx *ctx, uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, uint8_t *ok, const uint8_t *y,
                             const uint8_t *r, const uint8_t *data, const uint32_t *data_off, size_t n, void *stream);
int lcb_tpke_encrypt_dev(uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, uint8_t *ok, const uint8_t *y, const uint8_t *r,
                         const uint8_t *data, const uint32_t *data_off, size_t n, void *stream);
/* PublicKey.FullDecrypt behind lcb_tpke_combine_dev / lcb_tpke_combine_ordered_dev: the same grouped arguments (order
   null: index order) plus the ciphertexts' V; pt_out item c = V_c ^ KDF(u_c), packed as v_data, zero bytes where
   status[c] = 0 (fewer than k accepted shares, a repeated position). */
int lcb_ctx_tpke_full_decrypt_dev(lcb_ctx *ctx, uint8_t *pt_out, uint8_t *status, const uint8_t *accept,
                                  const uint8_t *shares, const uint32_t *order, size_t per_ct, size_t k,
                                  const uint8_t *v_data, const uint32_t *v_off, size_t n_cts, void *stream);
int lcb_tpke_full_decrypt_dev(uint8_t *pt_out, uint8_t *status, const uint8_t *accept, const uint8_t *shares,
                              const uint32_t *order, size_t per_ct, size_t k, const uint8_t *v_data,
                              const uint32_t *v_off, size_t n_cts, void *stream);
/* PublicKey.FullDecrypt literally (TPKE/PublicKey.cs:74-84) for a batch: problem j combines ALL its entries
   off[j] .. off[j + 1) (share uis[e] at x = ids[e] + 1) and opens V_j; status as lcb_g1_lagrange_batch (0 for a repeated
   id), pt_out item j zero bytes where status[j] = 0.  The count and share-id checks are the caller's. */
int lcb_tpke_full_decrypt_batch(uint8_t *pt_out, uint8_t *status, const int32_t *ids, const uint8_t *uis,
                                const uint32_t *off, const uint8_t *v_data, const uint32_t *v_off, size_t n_cts);
/* kernel milliseconds of k_kdf_xor in the last keystream call (any of the above) of the context (null: the calling
   thread's *_dev context) / of the calling thread's host-pointer forms; waits for that call */
int lcb_ctx_kdf_phase_ms(lcb_ctx *ctx, float ms[1]);
int lcb_kdf_phase_ms(float ms[1]);

#ifdef __cplusplus
}
#endif
#endif
