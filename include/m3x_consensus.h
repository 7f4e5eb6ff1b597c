/* m3x_consensus — C-ABI of the MI355X-native consensus hot-path library.
 *
 * This is the FFI boundary a Lighthouse-class host binds against (see
 * INTEGRATION.md for the Rust-side binding). Each entry point cites the
 * reference interface it replaces:
 *
 *  - m3x_bls_verify_sets        <- crypto/bls/src/impls/blst.rs:37-119
 *                                  (bls::verify_signature_sets; the batch
 *                                  equation with host-drawn 64-bit r_i)
 *  - m3x_bls_verify_each        <- generic_signature_set.rs:111-120
 *                                  (SignatureSet::verify, once per set: the
 *                                  gossip drivers' batch-false fallback)
 *  - m3x_bls_pk_decompress      <- blst.rs:130-153 key_validate, as used by
 *                                  validator_pubkey_cache.rs:20-46
 *  - m3x_merkleize_validators   <- BeaconState::update_validators_tree_hash_cache
 *                                  (consensus/types/src/beacon_state.rs:2043;
 *                                  List[Validator, 2^40], eth_spec.rs:404)
 *  - m3x_merkleize_chunks       <- tree_hash merkle_root + mix_in_length
 *                                  (merkle_proof/src/lib.rs:68-100,
 *                                  deposit_data_tree.rs:26-38)
 *  - m3x_kzgc_compute_cells,
 *    m3x_kzgc_verify_cell_proof_batch,
 *    m3x_kzgc_recover_cells
 *                               <- crypto/kzg/src/lib.rs:171-216 (the PeerDAS
 *                                  cell functions, stubbed TODO(das) there)
 *
 * Conventions: plain pointers + sizes, caller-owned host buffers,
 * synchronous calls (internally pipelined H2D/compute), errors as negative
 * codes, verification failure is 0 (false) — never an error (the
 * crypto/bls lib.rs:49-62 contract). The *_dev variants take device
 * pointers obtained from m3x_dev_alloc/m3x_h2d so callers can keep inputs
 * resident in HBM across calls. All functions are thread-safe w.r.t.
 * distinct contexts; one context serializes on its own stream.
 */
#ifndef M3X_CONSENSUS_H
#define M3X_CONSENSUS_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct m3x_ctx m3x_ctx;

/* error codes */
#define M3X_OK 0
#define M3X_ERR_HIP -1      /* HIP runtime failure */
#define M3X_ERR_ARG -2      /* bad argument */
#define M3X_ERR_NOMEM -3
#define M3X_ERR_ENCODING -4 /* malformed point / non-canonical field element
                               (c_kzg::Error analogue) */

int32_t m3x_ctx_create(m3x_ctx **out, int32_t device);
void m3x_ctx_destroy(m3x_ctx *ctx);
/* version/capability probe (also serves as a loadability check) */
int32_t m3x_abi_version(void);

/* per-kernel HIP-event timing (for benchmarks/roofline): enable resets the
 * accumulators; kernel ids are the M3X_K_* slots (0 leaves, 1 reduce,
 * 2 finalize, 3 bls_prepare, 4 bls_h2c, 5 bls_miller, 6 bls_reduce,
 * 7 bls_finish, 8 bls_agg, 9 kzg_challenge, 10 kzg_decomp, 11 kzg_eval,
 * 12 kzg_batch_r, 13 kzg_mults, 14 kzg_reduce, 15 kzg_finish,
 * 16 kzgp_quotient, 17 kzgp_msm, 18 kzgp_finish, 19 bls_sigpair,
 * 20 bls_each: the per-set pairing kernel of m3x_bls_verify_each,
 * 21 kzgc_ntt: the three transform passes of m3x_kzgc_compute_cells,
 * 22 kzgc_decode: canonical check of the cell evaluations, 23 kzgc_combine:
 * challenge powers, row weights and the per-column interpolation,
 * 24 kzgc_recover: the vanishing values and the five transform passes of
 * m3x_kzgc_recover_cells, 26 bls_sigmsm: the batch signature sum as a
 * bucket MSM; where it runs, 19 times the signature pairing alone,
 * 27 kzgc_toeplitz: the coefficient pass and the fixed-base Toeplitz sums
 * of the cell proofs, 28 kzgc_proof_dft: their 128-point G1 transform and
 * compression (the cells of a cells-and-proofs call count into 21, the
 * recovery of a recover-and-proofs call into 24). 25 is
 * not a slot and stays M3X_ERR_ARG: it was the first id past the table
 * when the table had 25 entries and is probed as such. Cell
 * verification also counts into 10, 13, 14 and 15, whose work it shares). */
int32_t m3x_timing_enable(m3x_ctx *ctx, int32_t on);
int32_t m3x_kernel_ms(m3x_ctx *ctx, int32_t kernel_id, double *ms,
                      uint64_t *launches);

/* carry a 32B subtree root from `from_level` to `to_depth` against the
 * zero ladder, then optionally mix_in_length — the multi-GPU cap-finishing
 * primitive paired with m3x_validator_subtree_root_dev. The ladder holds
 * Z[0..64]: to_depth > 64 is M3X_ERR_ARG. */
int32_t m3x_finalize_root(m3x_ctx *ctx, const uint8_t node[32],
                          uint32_t from_level, uint32_t to_depth,
                          int64_t mix_len, uint8_t out_root[32]);

/* ---- device buffer management (for *_dev calls / benchmarks) ---- */
int32_t m3x_dev_alloc(m3x_ctx *ctx, uint64_t bytes, void **dev_ptr);
int32_t m3x_dev_free(m3x_ctx *ctx, void *dev_ptr);
int32_t m3x_h2d(m3x_ctx *ctx, void *dst_dev, const void *src_host,
                uint64_t bytes);
int32_t m3x_d2h(m3x_ctx *ctx, void *dst_host, const void *src_dev,
                uint64_t bytes);

/* ---- SHA256 SSZ merkleize (hot path #2) ---- */

/* hash_tree_root of List[Validator, 2^40] from packed 121-byte SSZ records
 * (validator.rs:25-35 layout), including the mix_in_length. */
int32_t m3x_merkleize_validators(m3x_ctx *ctx, const uint8_t *ssz, uint64_t n,
                                 uint8_t out_root[32]);
int32_t m3x_merkleize_validators_dev(m3x_ctx *ctx, const void *ssz_dev,
                                     uint64_t n, uint8_t out_root[32]);

/* merkleize n_chunks 32-byte chunks into a depth-`depth` tree (capacity
 * 2^depth, zero-ladder padded); if mix_len >= 0, mix_in_length(mix_len).
 * Caller zero-pads the tail chunk. depth > 64 or n_chunks > 2^depth is
 * M3X_ERR_ARG. */
int32_t m3x_merkleize_chunks(m3x_ctx *ctx, const uint8_t *chunks,
                             uint64_t n_chunks, uint32_t depth,
                             int64_t mix_len, uint8_t out_root[32]);
int32_t m3x_merkleize_chunks_dev(m3x_ctx *ctx, const void *chunks_dev,
                                 uint64_t n_chunks, uint32_t depth,
                                 int64_t mix_len, uint8_t out_root[32]);

/* Partial subtree root over n validator records at fixed subtree depth
 * (no zero-cap to 2^40, no length mix) — the multi-GPU shard primitive:
 * rank i computes its contiguous range's depth-d subtree root, rank 0
 * finishes with m3x_merkleize_chunks over the gathered roots. */
int32_t m3x_validator_subtree_root_dev(m3x_ctx *ctx, const void *ssz_dev,
                                       uint64_t n, uint32_t depth,
                                       uint8_t out_root[32]);

/* ---- incremental registry merkleize (SURVEY §8f.3 — the milhouse-style
 * cached rehash: beacon_state.rs:1990-2021 has_pending_updates path).
 * The cache holds every tree level in HBM; an update rehashes only the
 * dirty leaves and their root paths. ---- */
typedef struct m3x_registry_cache m3x_registry_cache;

/* build the cache from n packed 121-byte records; capacity is the next
 * power of two >= max(n, 256) (appends beyond it are an error this round). */
int32_t m3x_registry_cache_create(m3x_ctx *ctx, const uint8_t *ssz,
                                  uint64_t n, m3x_registry_cache **out);
void m3x_registry_cache_destroy(m3x_registry_cache *cache);
/* current List[Validator, 2^40] root (zero-cap + mix_in_length) */
int32_t m3x_registry_cache_root(m3x_ctx *ctx, m3x_registry_cache *cache,
                                uint8_t out_root[32]);
/* apply m updated/appended records at `indices` (each < capacity;
 * n grows to max over indices+1) and return the new root. m > 65536 or an
 * index >= capacity is M3X_ERR_ARG; a rejected call changes nothing: tree
 * and length stay as they were. */
int32_t m3x_registry_cache_update(m3x_ctx *ctx, m3x_registry_cache *cache,
                                  const uint64_t *indices,
                                  const uint8_t *recs /* m*121 */, uint64_t m,
                                  uint8_t out_root[32]);

/* Batched small-container merkleize: element i owns chunks
 * [offsets[i], offsets[i+1]) (0..32 chunks each); out_roots[i] = its
 * hash_tree_root (depth = ceil_log2(count); an empty group gives the zero
 * chunk). One launch for the BeaconState's many tiny containers.
 * M3X_ERR_ARG, before anything is launched, for n_elems == 0, a group of
 * more than 32 chunks or offsets that decrease. */
int32_t m3x_merkleize_batch(m3x_ctx *ctx, const uint8_t *chunks,
                            const uint32_t *offsets, uint64_t n_elems,
                            uint8_t *out_roots);

/* swap-or-not committee shuffle — restated from
 * consensus/swap_or_not_shuffle/src/shuffle_list.rs; in-place on u32
 * indices; rounds = ChainSpec::shuffle_round_count (90 mainnet,
 * chain_spec.rs:632); forwards semantics as the reference. */
int32_t m3x_shuffle_list(m3x_ctx *ctx, uint32_t *indices, uint64_t list_size,
                         uint32_t rounds, const uint8_t seed[32],
                         int32_t forwards);
int32_t m3x_shuffle_list_dev(m3x_ctx *ctx, void *indices_dev,
                             uint64_t list_size, uint32_t rounds,
                             const uint8_t seed[32], int32_t forwards);

/* ---- BLS12-381 batched signature-set verification (hot path #1) ---- */

/* key_validate a batch of compressed pubkeys: decompress + infinity reject +
 * subgroup check; uncomp[i] valid iff status[i]==0. (pubkey cache build) */
/* RFC 9380 test entries (external-vector pinning; not on the hot path):
 * the same device expand/SSWU/isogeny/cofactor code as the verify
 * pipeline, parameterized by DST so the literal RFC appendix vectors
 * (QUUX DSTs) apply. out_uniform (256B, optional NULL) exposes the
 * expand_message_xmd output for the G2 suite's len_in_bytes=256. */
int32_t m3x_bls_expand_test(m3x_ctx *ctx, const uint8_t *msg,
                            uint32_t msg_len, const uint8_t *dst,
                            uint32_t dst_len, uint32_t len_in_bytes,
                            uint8_t *out);
int32_t m3x_bls_h2c_test(m3x_ctx *ctx, const uint8_t *msg, uint32_t msg_len,
                         const uint8_t *dst, uint32_t dst_len,
                         uint8_t out_uncomp[192], uint8_t out_uniform[256]);

/* Test entries for the hash-to-curve square roots (not on the hot path).
 * Fp2 elements are c0 || c1, 48-byte big-endian each; points are 192
 * uncompressed bytes (x.c1 || x.c0 || y.c1 || y.c0), all zero for infinity.
 * fp2_sqrt_test: one lane per element; ok[i] = 1 and out[i]^2 = a[i] for a
 *   square, ok[i] = 0 and out[i] = 0 otherwise.
 * sswu_test: per u, SSWU + 3-isogeny + to-affine, no cofactor clear.
 * h2c_batch_test: hash_to_curve of n 32-byte messages under the product DST
 *   through the pipeline's own kernels, cofactor cleared: mode 0 the fused
 *   kernel, mode 1 expand -> map -> fin, mode 2 their latency-regime twins. */
int32_t m3x_bls_fp2_sqrt_test(m3x_ctx *ctx, const uint8_t *a /* n*96 */,
                              uint64_t n, uint8_t *out /* n*96 */,
                              uint8_t *ok /* n */);
int32_t m3x_bls_sswu_test(m3x_ctx *ctx, const uint8_t *u /* n*96 */,
                          uint64_t n, uint8_t *out /* n*192 */);
/* as sswu_test, every u through the exceptional-input branch (sswu_g2_slow) */
int32_t m3x_bls_sswu_slow_test(m3x_ctx *ctx, const uint8_t *u /* n*96 */,
                               uint64_t n, uint8_t *out /* n*192 */);
int32_t m3x_bls_h2c_batch_test(m3x_ctx *ctx, const uint8_t *msgs /* n*32 */,
                               uint64_t n, int32_t mode,
                               uint8_t *out /* n*192 */);

/* Test entry for the batch pipeline's signature sum: decompresses the n
 * signatures, forms sum_i rands[i] * sigs[i] with the bucket MSM
 * (use_msm != 0) or with the per-set multiplications and the two-stage
 * reduction (use_msm == 0), and writes the sum as an uncompressed affine
 * point. Returns 0, or 1 for a sum at infinity (out_uncomp all zero);
 * M3X_ERR_ENCODING if a signature does not decode. No subgroup check. */
int32_t m3x_bls_sig_sum_test(m3x_ctx *ctx, const uint8_t *sigs /* n*96 */,
                             const uint64_t *rands /* n */, uint64_t n,
                             int32_t use_msm, uint8_t out_uncomp[192]);

int32_t m3x_bls_pk_decompress(m3x_ctx *ctx, const uint8_t *comp /* n*48 */,
                              uint64_t n, uint8_t *uncomp /* n*96 */,
                              int32_t *status /* n */);

/* The blst.rs:37-119 batch check over n signature sets:
 *   msgs: n*32 (signing roots); sigs: n*96 compressed G2 (SSZ wire form;
 *   decompressed on-GPU, subgroup checks deferred to here exactly as
 *   generic_aggregate_signature.rs:161-176 + blst.rs:73-77);
 *   pks: sum(k_i)*96 uncompressed affine G1, ALREADY validated once at
 *   cache build (validator_pubkey_cache model); pk_offsets: n+1;
 *   rands: n host-drawn 64-bit nonzero scalars (blst.rs:53-68).
 * Host-side rules the caller keeps (as the reference keeps them above
 * blst): empty set list, empty (all-zero) signatures, empty key lists.
 * Returns 1 valid / 0 invalid / <0 error. */
/* Aggregate n compressed G2 signatures into one (the TAggregateSignature
 * add_assign surface, generic_aggregate_signature.rs:124-150; used by
 * attestation aggregation). Invalid encodings -> nonzero return; the sum
 * may legitimately be the point at infinity (0xc0...). */
int32_t m3x_bls_sig_aggregate(m3x_ctx *ctx, const uint8_t *sigs /* n*96 */,
                              uint64_t n, uint8_t out_sig[96]);

int32_t m3x_bls_verify_sets(m3x_ctx *ctx, const uint8_t *msgs,
                            const uint8_t *sigs, const uint8_t *pks,
                            const uint32_t *pk_offsets, const uint64_t *rands,
                            uint64_t n);
int32_t m3x_bls_verify_sets_dev(m3x_ctx *ctx, const void *msgs_dev,
                                const void *sigs_dev, const void *pks_dev,
                                const void *pk_offsets_dev,
                                const void *rands_dev, uint64_t n);

/* SignatureSet::verify() for each of n sets, one call: verdicts[i] = 1/0
 * (generic_signature_set.rs:111-120 -> fast_aggregate_verify,
 * blst.rs:250-261; what the gossip drivers fall back to when a batch is
 * false, attestation_verification/batch.rs:109-127 and :195). No
 * randomiser: verdict_i = 1 iff sigma_i decodes, is in the G2 subgroup
 * (infinity counts as in), k_i >= 1, every pubkey of the set parses, their
 * sum apk_i is not infinity and
 *   final_exp(miller(apk_i, H(m_i)) * miller(-g1, sigma_i)) == 1.
 * Same input layout as m3x_bls_verify_sets, without rands. Returns M3X_OK
 * (n == 0 included, nothing written) or a negative error; an invalid set
 * is verdict 0, never an error, and never changes another set's verdict.
 * k_i == 0 (pk_offsets[i+1] <= pk_offsets[i]) is verdict 0 for that set. */
int32_t m3x_bls_verify_each(m3x_ctx *ctx, const uint8_t *msgs,
                            const uint8_t *sigs, const uint8_t *pks,
                            const uint32_t *pk_offsets, uint64_t n,
                            int32_t *verdicts /* n */);
int32_t m3x_bls_verify_each_dev(m3x_ctx *ctx, const void *msgs_dev,
                                const void *sigs_dev, const void *pks_dev,
                                const void *pk_offsets_dev, uint64_t n,
                                void *verdicts_dev /* n * int32 */);

/* ---- KZG blob proof verification (Deneb; crypto/kzg/src/lib.rs) ----
 *
 * Big-endian everywhere: commitments/proofs are 48B compressed G1 (infinity
 * 0xc0... is valid), z/y are 32B canonical scalars, a blob is 4096 x 32B
 * canonical scalars. Verify calls return 1 valid / 0 invalid / <0 error; a
 * failed proof is 0, never an error. A malformed point, a point outside
 * the subgroup or a scalar >= r is M3X_ERR_ENCODING. n == 0 returns 1.
 * The check is the batch equation
 *   e(sum r^i pi_i, -[tau]G2) *
 *   e(sum r^i (C_i - y_i G1) + sum r^i z_i pi_i, G2) == 1
 * with r from the spec's RCKZGBATCH___V1_ transcript (n == 1 included). */
typedef struct m3x_kzg m3x_kzg;

/* Kzg::new_from_trusted_setup (lib.rs:62-70), verification part only: the
 * one setup point verification needs is [tau]G2 = g2_monomial[1], 96B
 * compressed. Validated on the device (on curve, in the subgroup, not
 * infinity; else M3X_ERR_ENCODING); -[tau]G2 stays in device memory. */
int32_t m3x_kzg_create(m3x_ctx *ctx, const uint8_t g2_tau[96],
                       m3x_kzg **out);
void m3x_kzg_destroy(m3x_kzg *kzg);

/* Kzg::verify_kzg_proof (lib.rs:152-167) */
int32_t m3x_kzg_verify_proof(m3x_ctx *ctx, m3x_kzg *kzg, const uint8_t c[48],
                             const uint8_t z[32], const uint8_t y[32],
                             const uint8_t proof[48]);
/* verify_kzg_proof_batch of the spec (what lib.rs:105-132 reaches inside
 * c-kzg once z, y are known): cs/proofs n*48, zs/ys n*32 */
int32_t m3x_kzg_verify_proof_batch(m3x_ctx *ctx, m3x_kzg *kzg,
                                   const uint8_t *cs, const uint8_t *zs,
                                   const uint8_t *ys, const uint8_t *proofs,
                                   uint64_t n);
/* Kzg::verify_blob_kzg_proof (lib.rs:83-103) with n == 1 and
 * Kzg::verify_blob_kzg_proof_batch (lib.rs:105-132): blobs n*131072 */
int32_t m3x_kzg_verify_blob_proof_batch(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const uint8_t *blobs,
                                        const uint8_t *cs,
                                        const uint8_t *proofs, uint64_t n);
/* same, all three inputs already in device memory */
int32_t m3x_kzg_verify_blob_proof_batch_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                            const void *blobs_dev,
                                            const void *cs_dev,
                                            const void *proofs_dev,
                                            uint64_t n);

/* ---- KZG commitments and proofs ("KZG prover"; crypto/kzg/src/lib.rs) ----
 *
 * The producing half of the Kzg wrapper, on the m3x_kzg handle above. Every
 * result is sum_i s_i * L_i over the setup's 4096 Lagrange points: a
 * fixed-base multi-scalar multiplication served from a precomputed table of
 * [d * 16^j] L_i (d = 1..8, j = 0..63; about 200 MB of device memory per
 * handle). Calls return 0 on success (n == 0 included), M3X_ERR_ENCODING
 * for a non-canonical blob element or z, or a bad commitment, and
 * M3X_ERR_ARG on a handle that has no Lagrange basis loaded. */

/* Kzg::new_from_trusted_setup (lib.rs:62-70), the g1_lagrange part: 4096 x
 * 48B compressed points in the ceremony file's order (the bit-reversal
 * permutation is applied inside, as c-kzg does). Every point is validated
 * on the device (decodes, in the subgroup, not infinity; else
 * M3X_ERR_ENCODING and the handle stays verification-only), then the table
 * is built once and lives as long as the handle. One load per handle. */
int32_t m3x_kzgp_load_g1_lagrange(m3x_ctx *ctx, m3x_kzg *kzg,
                                  const uint8_t *g1_lagrange /* 4096*48 */);

/* Kzg::blob_to_kzg_commitment (lib.rs:134-139), n blobs in one call:
 * blobs n*131072 -> out n*48 */
int32_t m3x_kzgp_blob_to_commitment(m3x_ctx *ctx, m3x_kzg *kzg,
                                    const uint8_t *blobs, uint64_t n,
                                    uint8_t *out);
/* Kzg::compute_kzg_proof (lib.rs:141-150): blobs n*131072, zs n*32 ->
 * proofs_out n*48 and ys_out n*32 (y_i = p_i(z_i)); z inside the
 * evaluation domain takes the spec's in-domain quotient term */
int32_t m3x_kzgp_compute_proof(m3x_ctx *ctx, m3x_kzg *kzg,
                               const uint8_t *blobs, const uint8_t *zs,
                               uint64_t n, uint8_t *proofs_out,
                               uint8_t *ys_out);
/* Kzg::compute_blob_kzg_proof (lib.rs:72-81): blobs n*131072, cs n*48
 * (validated like any KZG point; infinity is valid) -> out n*48 */
int32_t m3x_kzgp_compute_blob_proof(m3x_ctx *ctx, m3x_kzg *kzg,
                                    const uint8_t *blobs, const uint8_t *cs,
                                    uint64_t n, uint8_t *out);
/* the same three with every input and output in device memory */
int32_t m3x_kzgp_blob_to_commitment_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const void *blobs_dev, uint64_t n,
                                        void *out_dev);
int32_t m3x_kzgp_compute_proof_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                   const void *blobs_dev, const void *zs_dev,
                                   uint64_t n, void *proofs_out_dev,
                                   void *ys_out_dev);
int32_t m3x_kzgp_compute_blob_proof_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const void *blobs_dev,
                                        const void *cs_dev, uint64_t n,
                                        void *out_dev);

/* test/introspection seams (like m3x_bls_h2c_test; not on the hot path).
 * blob_challenge_eval: z_i = compute_challenge(blob_i, c_i) (or zs_in[i]
 * when zs_in != NULL) and y_i = blob_i's polynomial at z_i; out_z/out_y
 * n*32. batch_challenge_test: the verify_kzg_proof_batch challenge r. */
int32_t m3x_kzg_blob_challenge_eval(m3x_ctx *ctx, const uint8_t *blobs,
                                    const uint8_t *cs, const uint8_t *zs_in,
                                    uint64_t n, uint8_t *out_z,
                                    uint8_t *out_y);
int32_t m3x_kzg_batch_challenge_test(m3x_ctx *ctx, const uint8_t *cs,
                                     const uint8_t *zs, const uint8_t *ys,
                                     const uint8_t *proofs, uint64_t n,
                                     uint8_t out_r[32]);

/* ---- PeerDAS cell KZG (Fulu; the seam crypto/kzg/src/lib.rs:171-216 stubs
 * with TODO(das): compute_cells_and_proofs, verify_cell_proof_batch,
 * cells_to_blob, recover_all_cells) ----
 *
 * A cell is 64 x 32B canonical big-endian scalars (2048 B); a blob extends
 * to 128 cells. With omega_N = 7^((r-1)/N), cell c holds the blob
 * polynomial's values on the coset h_c * <omega_64>, h_c =
 * omega_8192^bitrev7(c), element i at h_c * omega_64^bitrev6(i): the
 * bit-reversed 8192-point domain, so cells 0..63 are the blob itself
 * (cells_to_blob, lib.rs:203-206, is their concatenation and needs no call).
 * m3x_kzgc_compute_cells gives the cells alone and needs no setup;
 * m3x_kzgc_compute_cells_and_proofs further down gives both halves of
 * lib.rs:171-185 and needs the g1_monomial table. */

/* The cells of lib.rs:171-185: blobs n*131072 -> cells_out n*128*2048; needs
 * no setup. M3X_ERR_ENCODING for a non-canonical element; n == 0 is M3X_OK,
 * nothing written; n > 65535 is M3X_ERR_ARG. */
int32_t m3x_kzgc_compute_cells(m3x_ctx *ctx, const uint8_t *blobs, uint64_t n,
                              uint8_t *cells_out);
int32_t m3x_kzgc_compute_cells_dev(m3x_ctx *ctx, const void *blobs_dev,
                                  uint64_t n, void *cells_out_dev);

/* The two setup inputs cell verification needs: g1_monomial[0..64) (64*48 B)
 * and g2_monomial[64] = [tau^64]G2 (96 B). Validated on the device (decodes,
 * in the subgroup, not infinity; else M3X_ERR_ENCODING and the handle is
 * unchanged). One load per handle: a second one is M3X_ERR_ARG. */
int32_t m3x_kzgc_load_cell_setup(m3x_ctx *ctx, m3x_kzg *kzg,
                                const uint8_t *g1_monomial64,
                                const uint8_t g2_tau64[96]);

/* Kzg::verify_cell_proof_batch (lib.rs:187-201): n cells, cell k at
 * (rows[k], cols[k]) of the blob matrix with proof k, against commitment
 * rows[k] of m. 1 valid / 0 invalid / <0 error; n == 0 returns 1.
 * M3X_ERR_ARG, before any launch: handle without cell setup, row >= m,
 * col >= 128, m == 0 with n > 0, n > 65535. M3X_ERR_ENCODING: bad point,
 * point outside the subgroup, evaluation >= r. The check is
 *   e(sum r^k pi_k, -[tau^64]G2) *
 *   e(sum_i w_i C_i - sum_j a_j [tau^j]G1 + sum r^k h_col^64 pi_k, G2) == 1
 * with w_i the sum of r^k over row i, a_j coefficient j of sum r^k I_k (I_k
 * the degree < 64 interpolant of cell k), and r = hash_to_bls_field of
 *   "RCKZGCBATCH__V1_" | BE64(4096) | BE64(64) | BE64(m) | BE64(n) |
 *   commitments | per cell: BE64(row) BE64(col) cell proof.
 * There is no _dev form: the transcript is hashed on the calling thread
 * while the device validates the points, which needs the bytes on the host. */
int32_t m3x_kzgc_verify_cell_proof_batch(m3x_ctx *ctx, m3x_kzg *kzg,
                                        const uint8_t *commitments /* m*48 */,
                                        uint64_t m, const uint64_t *rows,
                                        const uint64_t *cols /* n each */,
                                        const uint8_t *cells /* n*2048 */,
                                        const uint8_t *proofs /* n*48 */,
                                        uint64_t n);

/* test seam, like m3x_kzg_batch_challenge_test: the challenge r only (host
 * work; takes no handle). n == 0 or an argument the verify call refuses is
 * M3X_ERR_ARG. */
int32_t m3x_kzgc_cell_batch_challenge_test(m3x_ctx *ctx,
                                          const uint8_t *commitments,
                                          uint64_t m, const uint64_t *rows,
                                          const uint64_t *cols,
                                          const uint8_t *cells,
                                          const uint8_t *proofs, uint64_t n,
                                          uint8_t out_r[32]);

/* Kzg::recover_all_cells (lib.rs:208-216), for n blobs that share one set of
 * known columns (a reconstructing node holds whole data columns): from k >= 64
 * of a blob's 128 cells, all 128. Blob b's known cell t is at
 * cells + (b*k + t)*2048 and is cell number cell_ids[t]; the ids may come in
 * any order, the output is always cells 0..127 in order. Needs no setup and
 * no m3x_kzg handle, like m3x_kzgc_compute_cells.
 * M3X_ERR_ARG, before any launch: k < 64, k > 128, an id >= 128, a repeated
 * id, n > 65535. n == 0 is M3X_OK and nothing is written (the argument checks
 * still apply). M3X_ERR_ENCODING: an evaluation >= r, or known cells that do
 * not lie on one polynomial of degree < 4096 (possible only when k > 64; the
 * check is exact: the recovered quotient's coefficients 4096..8191 must all
 * be zero, and then it agrees with every known cell). On an error the output
 * buffer's contents are unspecified; the context stays usable.
 * Method: the spec's recover_polynomialcoeff, the vanishing polynomial of the
 * missing cells taken by its 128 values per domain instead of being formed;
 * three 8192-point transforms and the forward half of compute_cells. The
 * proofs come from m3x_kzgc_recover_cells_and_proofs. */
int32_t m3x_kzgc_recover_cells(m3x_ctx *ctx, const uint64_t *cell_ids, uint64_t k,
                               const uint8_t *cells /* n*k*2048, blob-major */,
                               uint64_t n, uint8_t *cells_out /* n*128*2048 */);
int32_t m3x_kzgc_recover_cells_dev(m3x_ctx *ctx, const uint64_t *cell_ids /* host */,
                                   uint64_t k, const void *cells_dev, uint64_t n,
                                   void *cells_out_dev);

/* ---- PeerDAS cell proofs (Kzg::compute_cells_and_proofs,
 * crypto/kzg/src/lib.rs:171-185, the proof half; the spec's
 * compute_cells_and_kzg_proofs and recover_cells_and_kzg_proofs) ----
 *
 * The proof of cell c is [q_c(tau)]G1, q_c = p // (X^64 - y_c) with p the
 * blob's coefficient list and y_c = h_c^64 = omega_128^bitrev7(c). Method:
 *   h_m     = sum_j p[j + 64(m+1)] * g1_monomial[j]     m = 0..62
 *   proof_c = sum_m y_c^m * h_m                         c = 0..127
 * the 63 sums h_m straight from a fixed-base table over g1_monomial (signed
 * 4-bit digits, look-ups joined by mixed additions, no doublings), then one
 * 128-point G1 transform per blob and compression. */

/* lib.rs:171-185 needs the whole g1_monomial list: 4096 x 48B compressed
 * points in the ceremony file's order (natural order: entry j is
 * [tau^j]G1). Every point is validated on the device (decodes, in the
 * subgroup, not infinity; else M3X_ERR_ENCODING and the handle is
 * unchanged), then the table of [d * 16^j] multiples is built once: about
 * 200 MB more of device memory per handle (4096 bases, of which the sums
 * use 4032), freed by m3x_kzg_destroy. One load per handle: a second one is
 * M3X_ERR_ARG. Independent of m3x_kzgp_load_g1_lagrange and
 * m3x_kzgc_load_cell_setup. */
int32_t m3x_kzgc_load_g1_monomial(m3x_ctx *ctx, m3x_kzg *kzg,
                                 const uint8_t *g1_monomial /* 4096*48, file order */);

/* lib.rs:171-185, n blobs in one call: blobs n*131072 -> cells_out
 * n*128*2048 (may be NULL: proofs only) and proofs_out n*128*48, the proof
 * of blob b, cell c at (b*128 + c)*48. With cells_out the cells are
 * bit-identical to m3x_kzgc_compute_cells. M3X_ERR_ARG, before any launch:
 * handle without the monomial table, n > 65535, handle of another device.
 * M3X_ERR_ENCODING: a blob element >= r. n == 0 is M3X_OK, nothing written.
 * On an error the outputs are unspecified; the context stays usable. */
int32_t m3x_kzgc_compute_cells_and_proofs(m3x_ctx *ctx, m3x_kzg *kzg,
                                         const uint8_t *blobs, uint64_t n,
                                         uint8_t *cells_out,
                                         uint8_t *proofs_out);
int32_t m3x_kzgc_compute_cells_and_proofs_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                             const void *blobs_dev, uint64_t n,
                                             void *cells_out_dev,
                                             void *proofs_out_dev);

/* recover_cells_and_kzg_proofs (the proof half lib.rs:208-216 leaves out):
 * m3x_kzgc_recover_cells as it stands, then the proof pipeline over the
 * recovered blobs, which are cells 0..63 of each output, read in place.
 * Every argument and error rule of m3x_kzgc_recover_cells applies and is
 * checked first, then the rules of m3x_kzgc_compute_cells_and_proofs.
 * cells_out n*128*2048 (required), proofs_out n*128*48. */
int32_t m3x_kzgc_recover_cells_and_proofs(m3x_ctx *ctx, m3x_kzg *kzg,
                                         const uint64_t *cell_ids, uint64_t k,
                                         const uint8_t *cells /* n*k*2048 */,
                                         uint64_t n, uint8_t *cells_out,
                                         uint8_t *proofs_out);
int32_t m3x_kzgc_recover_cells_and_proofs_dev(m3x_ctx *ctx, m3x_kzg *kzg,
                                             const uint64_t *cell_ids /* host */,
                                             uint64_t k, const void *cells_dev,
                                             uint64_t n, void *cells_out_dev,
                                             void *proofs_out_dev);

#ifdef __cplusplus
}
#endif
#endif
