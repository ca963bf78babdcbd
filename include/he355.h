/*
 * he355.h — C ABI of the MI355X hot path ("thin extern C FFI" of the backend).
 *
 * These are the entry points a host in any language binds (cgo / JNI / ctypes / the C++ HEBench classes in
 * reference-seal-backend_amd/csrc/bridge) in place of the seal::Evaluator calls the reference makes inside its
 * timed operate() bodies.  Plain pointers and sizes only; no C++ or torch types.  All `d_*` pointers are
 * device (HBM) pointers obtained from he355_malloc; ciphertext slabs are arrays of SEAL-layout ciphertexts
 * [n][size][L][N] of uint64 residues (CKKS: NTT form), i.e. byte-compatible with seal::Ciphertext::data().
 *
 * Reference interface replaced (file:line under /root/reference):
 *   he355_ctx_create            SEALContextWrapper::createCKKSContext/createBFVContext  include/engine/seal_context.h:32-50,
 *                               parameter rule src/engine/seal_context.cpp:79-90,107-119
 *   he355_set_relin_key         KeyGenerator::create_relin_keys                         src/engine/seal_context.cpp:53
 *   he355_set_galois_key        KeyGenerator::create_galois_keys                        src/engine/seal_context.cpp:69
 *   he355_add                   evaluator()->add          src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:340,
 *                                                         src/benchmarks/bfv/seal_bfv_element_wise_benchmark.cpp:322
 *   he355_multiply              evaluator()->multiply     src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:343
 *   he355_multiply_relin        multiply + relinearize_inplace                src/benchmarks/ckks/seal_ckks_dot_product_benchmark.cpp:325-329
 *     (rescale = 1)             ... + rescale_to_next_inplace                 src/benchmarks/ckks/seal_ckks_matmultval_benchmark.cpp:253-255
 *   he355_relinearize           evaluator()->relinearize_inplace              src/engine/seal_context.cpp:390,447
 *   he355_multiply_accumulate   multiply + add_inplace over the inner dimension  src/benchmarks/ckks/seal_ckks_matmult_cipherbatchaxis_benchmark.cpp:404-420
 *   he355_relinearize_rescale   relinearize_inplace + rescale_to_next_inplace    same file :436-437
 *   he355_bfv_multiply_relin_accumulate  multiply + relinearize_inplace + add_inplace over the inner dimension
 *                                                         src/benchmarks/bfv/seal_bfv_matmult_cipherbatchaxis_benchmark.cpp:398-410
 *   he355_rescale               evaluator()->rescale_to_next_inplace          src/engine/seal_context.cpp:391,448
 *   he355_rotate                evaluator()->rotate_vector (CKKS) / rotate_rows (BFV)      src/engine/seal_context.cpp:337,302
 *   he355_apply_galois(2N-1)    evaluator()->rotate_columns_inplace (BFV)                   src/engine/seal_context.cpp:308
 *   he355_accumulate            SEALContextWrapper::accumulateCKKS / accumulateBFV          src/engine/seal_context.cpp:321-347,289-319
 *   the Indexer                 ParameterIndexer{value_index,batch_size} and the result order r = i*b1 + x
 *                                                         src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:322-336
 *
 * Error convention: every function returns 0 on success or a non-zero code (HE355_E_*); the message is kept
 * per thread and read with he355_last_error() — the same shape as the API Bridge's ErrorCode +
 * getLastErrorDescription.  There is NO CPU fallback: without a HIP device every device call fails with
 * HE355_E_DEVICE.
 */
#ifndef HE355_H
#define HE355_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HE355_SCHEME_BFV 1
#define HE355_SCHEME_CKKS 2

#define HE355_OK 0
#define HE355_E_INVALID_ARGS 1 /* same meaning as HEBENCH_ECODE_INVALID_ARGS   */
#define HE355_E_PARAMS 2       /* parameter/context error; the reference reports these as HEBSEAL_ECODE_SEAL_ERROR = 2 */
#define HE355_E_DEVICE 3       /* HIP error or no device                        */
#define HE355_E_CRITICAL 0x7FFFFFFF

typedef struct he355_ctx he355_ctx;

/* operand selection for result r of a batch (see the Indexer row above) */
typedef struct {
    uint64_t a_base, b_base; /* value_index of operand 0 / operand 1                  */
    uint64_t b1;             /* batch size of operand 1: a = a_base + r / b1, b = b_base + r % b1 */
    int32_t pairwise;        /* 1: a = a_base + r, b = b_base + r                     */
    int32_t reserved;
} he355_indexer;

const char *he355_last_error(void);

/* ---- context (host only; no HIP call is made until he355_device_init) ---- */
int he355_ctx_create(int scheme, uint64_t poly_modulus_degree, const int32_t *bit_sizes, uint64_t n_bit_sizes, int plain_modulus_bits,
                     int enforce_sec128, he355_ctx **out);
int he355_ctx_create_primes(int scheme, uint64_t poly_modulus_degree, const uint64_t *primes, uint64_t n_primes, uint64_t plain_modulus,
                            he355_ctx **out);
void he355_ctx_destroy(he355_ctx *ctx);
uint64_t he355_poly_degree(const he355_ctx *ctx);
uint64_t he355_key_modulus_count(const he355_ctx *ctx);  /* K, special prime last       */
uint64_t he355_data_modulus_count(const he355_ctx *ctx); /* L at the first data level   */
uint64_t he355_modulus(const he355_ctx *ctx, uint64_t i);
uint64_t he355_plain_modulus(const he355_ctx *ctx);
int he355_prime_uses_fp64(const he355_ctx *ctx, uint64_t i); /* which arithmetic engine owns prime i */
/* BFV: the auxiliary base of the BEHZ multiply at `level` data primes: out[0] = m_sk, out[1..] = B_0.. (at most cap entries written);
 * returns their number, 0 for CKKS or a bad level.  SEAL's RNSTool (seal/util/rns.cpp, RNSTool::initialize) takes 61-bit primes; the
 * product does not depend on the choice and the device takes primes of its fp64 engine (csrc/he_params.h, Params::aux). */
uint64_t he355_bfv_aux_base(const he355_ctx *ctx, int level, uint64_t *out, uint64_t cap);
uint32_t he355_galois_elt_from_step(const he355_ctx *ctx, int step);
uint64_t he355_galois_elts_all(const he355_ctx *ctx, uint32_t *out, uint64_t cap);

/* ---- device ---- */
int he355_device_count(int *count);
int he355_device_init(he355_ctx *ctx, int device_ordinal); /* uploads tables; creates the stream */
/* Device memory comes from the context's pool (csrc/device_pool.h): size-class free lists over hipMalloc'd blocks, the counterpart
 * of the MemoryPoolHandle::ThreadLocal() the reference hands to the evaluator inside operate()
 * (src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:343).  he355_free returns the block to its list: no HIP call and no
 * synchronisation (a re-issued block is only touched by work queued later on the context's streams), so a steady-state operate()
 * performs no hipMalloc / hipFree.  he355_alloc_stats counts every raw hipMalloc / hipFree the context has made since
 * he355_device_init (its tables, keys and scratch arenas included); he355_pool_trim drains the streams and hipFree()s the cached
 * blocks (also done by itself when the device runs out of memory). */
int he355_malloc(he355_ctx *ctx, uint64_t bytes, void **d_ptr);
/* he355_free takes ONLY pointers this context's he355_malloc returned and has not freed yet: a block freed twice, a pointer of another
 * context or one from hipMalloc is refused with HE355_E_INVALID_ARGS and left untouched (since round 5; before, a foreign pointer was
 * drained and hipFree()d).  A host that allocates device memory by other means must release it by the same means. */
int he355_free(he355_ctx *ctx, void *d_ptr);
typedef struct {
    uint64_t raw_mallocs, raw_frees; /* hipMalloc / hipFree calls            */
    uint64_t pool_hits, pool_misses;  /* he355_malloc served from a list / by a new block */
    uint64_t cached_bytes, live_bytes;
} he355_alloc_stats_t;
int he355_alloc_stats(he355_ctx *ctx, he355_alloc_stats_t *out); /* ctx == NULL: totals over every context of the process (byte fields 0) */
int he355_pool_trim(he355_ctx *ctx, uint64_t *released_bytes);
/* Which shape / schedule the context's key switches took since he355_device_init (or the last call with reset != 0).  The choice is the
 * library's (batch, ring size, level: DESIGN.md 5.2-5.3) and never changes a result bit; tests use the counters to prove that the shape they
 * mean to hold to the oracle is the one that ran (tests/test_gpu_bench_shapes.py).  A "sequence" is the kernel sequence of one chunk of a batch. */
typedef struct {
    uint64_t ks_fused;      /* throughput shape, mod-down finished inside k_k3                          */
    uint64_t ks_unfused;    /* throughput shape, separate floor kernels (small grids)                   */
    uint64_t ks_latency;    /* latency shape (digit-split tiles, batch x N <= 2^17)                     */
    uint64_t ks_lds;        /* ring-in-LDS shape (N <= 8192, few ciphertexts): one workgroup per residue polynomial */
    uint64_t level_sums_in_k3;         /* he355_rotate_sum levels whose sum was formed by k_k3 itself   */
    uint64_t level_sums_by_kernel;     /* ... by k_sum_groups                                            */
    uint64_t level_sum_launches_in_k3; /* fused sequences that carried a level sum (several per level when HE355_CHUNK cuts it) */
    uint64_t reserved;
} he355_path_stats_t;
int he355_path_stats(he355_ctx *ctx, he355_path_stats_t *out, int reset);
/* Which route the context's BFV PIR calls took since he355_device_init (or the last call with reset != 0).  The routes are the library's
 * (ring size, batch, strides: the ROUTED notes of DESIGN.md) and bit-identical by definition, so a result cannot tell which one ran; tests use
 * the counters to prove that the route they mean to hold to the oracle is the one that ran (tests/test_gpu_bfv_large_rings.py).  Counted on
 * the host where the calls branch; no counter is read by a launch.  A "pass" is one trip of he355_bfv_external_product or
 * he355_bfv_rgsw_from_bfv through its pool block of digit polynomials, or of one level of he355_bfv_select; that call's passes also count in
 * mac_gadget / mac_plain as the external product's do. */
typedef struct {
    uint64_t cut_cols, cut_stream;         /* cuts of he355_bfv_gadget_decompose_ntt and of he355_bfv_external_product's passes: the fused column pass / the streaming cut */
    uint64_t mac_gadget, mac_plain;        /* he355_bfv_external_product passes by multiply-accumulate kernel: k_bfv_gadget_mac / k_bfv_plain_mac */
    uint64_t own_cols, own_stream;         /* he355_bfv_rgsw_from_bfv passes by cut: the column pass that also emits the slot's own row / the streaming cut */
    uint64_t digits_fused, digits_routed;  /* he355_bfv_decompose_ntt calls: the fused column pass / N = 1024's composition */
    uint64_t bytes_fused, bytes_routed;    /* he355_bfv_unpack_bytes_ntt: fused calls / passes of N = 1024's composition through its pool block */
    uint64_t passes;                       /* pool-block passes of he355_bfv_external_product, he355_bfv_rgsw_from_bfv and he355_bfv_select */
    uint64_t select_cols, select_stream;   /* he355_bfv_select passes by cut: the column pass / the streaming cut, both of odd - even */
    uint64_t select_tail_fused, select_tail_routed; /* he355_bfv_select levels by tail: the inverse column pass that adds the even node / N = 1024's composition */
    uint64_t reserved[1];
} he355_bfv_route_stats_t;
int he355_bfv_route_stats(he355_ctx *ctx, he355_bfv_route_stats_t *out, int reset);
/* Which route the context's BEHZ multiplies (he355_bfv_multiply, he355_bfv_multiply_relin_accumulate) took since he355_device_init (or the
 * last call with reset != 0): DESIGN.md, "BFV multiply", lists the decisions.  Every route gives the same bits; tests use the counters to
 * prove which kernels they held to the oracle (tests/test_gpu_bfv_multiply_routes.py, against the restatement in tests/bfv_multiply_plan.py).
 * Counted on the host where the call branches; no counter is read by a launch. */
typedef struct {
    uint64_t calls_lists, calls_pairs;   /* calls by path: every distinct operand extended once / the two operands of every result */
    uint64_t chunks;                     /* kernel sequences over a chunk of results, both paths */
    uint64_t cols_fused, cols_unfused;   /* extensions and floor steps (one count each) with the column passes inside / as separate launches */
    uint64_t cols_exact;                 /* of cols_fused: the instantiations compiled for exactly L = nB = 2, 3, 4 at N = 8192 */
    uint64_t coef_wide;                  /* of cols_unfused: the <16, 24> coefficient kernels (L > 4 or nB > 6) */
    uint64_t rows_dual, rows_split;      /* per-pair chunks: k_behz_rows_tensor_dual / one launch per engine */
    uint64_t inv_dual, inv_split;        /* lists chunks: k_behz_tensor_inv_dual / one launch per engine */
    uint64_t lds_limit;                  /* not a counter: the dynamic LDS in bytes one block of the fused column kernels may ask for on this device */
    uint64_t reserved[4];
} he355_bfv_multiply_stats_t;
int he355_bfv_multiply_stats(he355_ctx *ctx, he355_bfv_multiply_stats_t *out, int reset);
int he355_upload(he355_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int he355_download(he355_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
int he355_copy(he355_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes); /* device to device, on the context's stream */
/* device memory of src_ctx's GPU -> device memory of dst_ctx's GPU (hipMemcpyPeer over xGMI; also valid when both contexts sit on the
 * same GPU).  Both contexts are synchronised first, the copy is complete on return.  Used at load() / store() by the bridge's
 * multi-device path: operand replicas out, result parts back; never inside operate(). */
int he355_copy_peer(he355_ctx *dst_ctx, void *d_dst, he355_ctx *src_ctx, const void *d_src, uint64_t bytes);
int he355_sync(he355_ctx *ctx);
/* synthetic data: fill n_polys residue polynomials with uniform residues, polynomial p using prime
 * prime_of[p % period] (throughput-mode inputs) */
int he355_fill_uniform(he355_ctx *ctx, uint64_t *d_dst, uint64_t n_polys, const uint8_t *prime_of, uint32_t period, uint64_t seed);
/* the same stream from polynomial `first_poly` on: a rank's shard of a batch holds what the whole batch would hold there */
int he355_fill_uniform_at(he355_ctx *ctx, uint64_t *d_dst, uint64_t n_polys, const uint8_t *prime_of, uint32_t period, uint64_t seed, uint64_t first_poly);

/* ---- evaluation keys: host arrays [L_top digits][2][K][N], NTT form (SEAL KSwitchKeys layout) ---- */
int he355_set_relin_key(he355_ctx *ctx, const uint64_t *h_key);
int he355_set_galois_key(he355_ctx *ctx, uint32_t galois_elt, const uint64_t *h_key);
/* KeyGenerator on the device (create_relin_keys / create_galois_keys, src/engine/seal_context.cpp:53,69) from the secret key given
 * to he355_set_secret_key; randomness: counter-based streams of `seed` (csrc/client/sampler.h keygen_stream) — the host client's
 * make_relin_key / make_galois_key with the same seed give the same bits */
int he355_keygen_relin(he355_ctx *ctx, uint64_t seed);
int he355_keygen_galois(he355_ctx *ctx, uint32_t galois_elt, uint64_t seed);
int he355_set_relin_key_synthetic(he355_ctx *ctx, uint64_t seed);                       /* uniform residues, generated in HBM */
int he355_set_galois_key_synthetic(he355_ctx *ctx, uint32_t galois_elt, uint64_t seed);

/* ---- batched evaluator ops on device slabs; L = residues at the operands' level ---- */
/* he355_add / he355_sub add residues whatever they stand for: also the add_inplace / sub_inplace of NTT-form BFV ciphertexts (below) */
int he355_add(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_a, const uint64_t *d_b, he355_indexer ix, uint64_t *d_out);
int he355_sub(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_a, const uint64_t *d_b, he355_indexer ix, uint64_t *d_out);
/* CKKS multiply: [.][2][L][N] x [.][2][L][N] -> [n][3][L][N] */
int he355_multiply(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_a, const uint64_t *d_b, he355_indexer ix, uint64_t *d_out);
/* BFV multiply (BEHZ, coefficient form): [.][2][L][N] x [.][2][L][N] -> [n][3][L][N]
 * (evaluator()->multiply, src/benchmarks/bfv/seal_bfv_element_wise_benchmark.cpp:325, seal_bfv_dot_product_benchmark.cpp:311).
 * In an outer-product batch every operand serves several results: each is extended to the auxiliary base and transformed once
 * (the values SEAL recomputes per pair), a result then costs its dyadic tensor, three inverse transforms and the floor.
 * d_out may not overlap an operand (HE355_E_INVALID_ARGS). */
int he355_bfv_multiply(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_a, const uint64_t *d_b, he355_indexer ix, uint64_t *d_out);
/* multiply -> relinearize (-> rescale): out [n][2][L][N] or [n][2][L-1][N].  Give d_out a slab of its own: then the tensor product's
 * c0, c1 never travel through HBM (the key-switch kernel forms them from the operand rows); a d_out that overlaps an operand is
 * detected and served by the slower path that materialises them first. */
int he355_multiply_relin(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_a, const uint64_t *d_b, he355_indexer ix, int rescale,
                         uint64_t *d_out);
int he355_relinearize(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_ct3, uint64_t *d_out);            /* [n][3][L][N] -> [n][2][L][N] */
/* CKKS plaintext operands: NTT-form plaintexts [.][L][N] at the ciphertexts' level; ciphertext r uses plaintext
 * b_base + r % b1 (or b_base + r when pairwise), ciphertext operand a_base + r / b1 (the Indexer rule).
 *   he355_multiply_plain: evaluator()->multiply_plain_inplace   src/engine/seal_context.cpp:390   (every polynomial x plain)
 *   he355_add_plain     : evaluator()->add_plain_inplace        src/engine/seal_context.cpp:454   (c0 += plain)        */
int he355_multiply_plain(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, const uint64_t *d_plain, he355_indexer ix, uint64_t *d_out);
int he355_add_plain(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, const uint64_t *d_plain, he355_indexer ix, uint64_t *d_out);
/* CKKS evaluator()->mod_switch_to_inplace / mod_switch_to_next_inplace (src/engine/seal_context.cpp:389,451 and matchLevel):
 * the last residues of every polynomial are dropped; in [n_polys][L][N] -> out [n_polys][L_to][N] (n_polys = n * size for
 * ciphertexts, n for plaintexts) */
int he355_mod_switch_drop(he355_ctx *ctx, int L, int L_to, uint64_t n_polys, const uint64_t *d_in, uint64_t *d_out);
/* ---- BFV level operations (BFV contexts only, else HE355_E_INVALID_ARGS; every L in 1..L_top).  Ciphertexts [n][size][L][N] in
 * coefficient form, size 1..3; plaintexts [.][N] coefficients mod t: what he355_bfv_encode writes and he355_encrypt reads.  Operands by
 * the Indexer rule of he355_multiply_plain: ciphertext a_base + r / b1, plaintext b_base + r % b1, or pairwise.
 * [UPSTREAM-UNVERIFIED] (SEAL is not part of this tree): the published SEAL v3.7.2 algorithms, SURVEY.md Appendix A.
 *   he355_bfv_mod_switch     Evaluator::mod_switch_to_next_inplace / mod_switch_to_inplace for BFV: L - L_to successive
 *                            RNSTool::divide_and_round_q_last_inplace steps, each dropping the current last prime with rounding, in ONE launch
 *                            (a polynomial is read once at L and written once at L_to residues).  -> [n][size][L_to][N]; 1 <= L_to <= L <= 16;
 *                            L_to == L copies.  d_out may not overlap d_in.
 *   he355_bfv_add_plain      Evaluator::add_plain_inplace / sub_plain_inplace (multiply_add/sub_plain_with_scaling_variant at the ciphertext's
 *   he355_bfv_sub_plain      level): c0 +- Delta_L(m), Delta_L(m) = floor((q_L m + floor((t + 1) / 2)) / t) mod q_i, q_L the product of the first
 *                            L primes; the other polynomials are copied.  d_out == d_ct is allowed exactly when every ciphertext serves one
 *                            result (pairwise, or b1 == 1); any other overlap is refused.
 *   he355_bfv_multiply_plain Evaluator::multiply_plain_inplace (multiply_plain_normal): every polynomial times lift(m) in Z_q_i[X]/(X^N + 1),
 *                            lift(m) = m below floor((t + 1) / 2), else m - t; canonical residues, coefficient form.  Each distinct plaintext
 *                            of the call is lifted and transformed once.  SEAL's optional "transparent ciphertext" exception is NOT reproduced:
 *                            a zero plaintext gives a zero ciphertext.  d_out may not overlap an operand. */
int he355_bfv_mod_switch(he355_ctx *ctx, int L, int L_to, int size, uint64_t n, const uint64_t *d_in, uint64_t *d_out);
int he355_bfv_add_plain(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, const uint64_t *d_plain, he355_indexer ix, uint64_t *d_out);
int he355_bfv_sub_plain(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, const uint64_t *d_plain, he355_indexer ix, uint64_t *d_out);
int he355_bfv_multiply_plain(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, const uint64_t *d_plain, he355_indexer ix, uint64_t *d_out);
/* ---- NTT-form BFV operands (BFV contexts only, else HE355_E_INVALID_ARGS, decided on the host before any device is asked for; every L in
 * 1..L_top; polynomial (k, i) of a ciphertext at level L is under prime i < L of the key chain).  SEAL's BFV evaluator has a second mode
 * for sums of plaintext products -- a plaintext matrix times an encrypted vector, a PIR database scan, a plain-weight linear layer: every
 * operand is transformed once, every term is a dyadic product and an addition, the result is transformed back once.
 * THE FORM OF A SLAB IS THE CALLER'S CONTRACT, as it is for CKKS: the library keeps raw slabs and does not track which form one is in.
 * The transforms use the bit order he355_ntt_forward uses.
 * [UPSTREAM-UNVERIFIED] as the level operations above (SEAL v3.7.2 evaluator.cpp):
 *   he355_bfv_transform_to_ntt    Evaluator::transform_to_ntt_inplace(Ciphertext &): [n][size][L][N], size 1..3, coefficient form -> NTT form.
 *   he355_bfv_transform_from_ntt  Evaluator::transform_from_ntt_inplace: the way back.  For both, d_out == d_in is allowed (in place); any
 *                                 other overlap is refused; n == 0 touches nothing.
 *   he355_bfv_plain_to_ntt        Evaluator::transform_to_ntt_inplace(Plaintext &, parms_id): d_plain [n][N] coefficients mod t -> d_out
 *                                 [n][L][N]: the centred lift he355_bfv_multiply_plain multiplies by (m below floor((t + 1) / 2), else m - t,
 *                                 reduced per prime), transformed under primes 0 .. L-1.  d_out may not overlap d_plain.
 *   he355_bfv_multiply_plain_ntt  Evaluator::multiply_plain on NTT-form operands (multiply_plain_ntt): every polynomial times the NTT-form
 *                                 plaintext, canonical residues; operands by the Indexer rule of he355_bfv_multiply_plain.  d_out == d_ct is
 *                                 allowed exactly when every ciphertext serves one result (pairwise, or b1 == 1), as in he355_bfv_add_plain;
 *                                 any other overlap is refused.  (he355_multiply_plain stays the CKKS entry and refuses BFV contexts.)
 *   he355_bfv_multiply_plain_accumulate
 *                                 out(i, j) = sum_{k < inner} ct(i, k) (.) pt(k, j), size-`size` results [rows * cols][size][L][N]: ciphertext
 *                                 (i, k) at index i * ct_stride_i + k * ct_stride_k, plaintext (k, j) at k * pt_stride_k + j * pt_stride_j (the
 *                                 addressing of he355_multiply_accumulate); size 1..3, inner 1..2^31-1; rows * cols == 0 returns without a
 *                                 launch; d_out may not overlap an operand.  One launch: the products are summed unreduced in 128 bits and
 *                                 reduced once per run (csrc/bfv_mac_core.h); the result is the canonical residue of the sum, bit-identical
 *                                 to the term-by-term multiply_plain + add_inplace loop.
 *   add_inplace / sub_inplace     he355_add / he355_sub: they are form-agnostic and serve NTT-form BFV ciphertexts as they are.
 * NOT for NTT-form BFV ciphertexts, as in SEAL 3.7.2 (which refuses them in multiply, relinearize, the rotations, mod_switch, add_plain and
 * decrypt): he355_bfv_multiply, he355_relinearize, he355_rotate / he355_apply_galois and their kin, he355_bfv_mod_switch,
 * he355_bfv_add_plain / sub_plain, he355_bfv_multiply_plain, he355_decrypt, he355_bfv_noise_budget.  Transform back first: the library
 * cannot check it and would compute garbage. */
int he355_bfv_transform_to_ntt(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_in, uint64_t *d_out);
int he355_bfv_transform_from_ntt(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_in, uint64_t *d_out);
int he355_bfv_plain_to_ntt(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain, uint64_t *d_out);
int he355_bfv_multiply_plain_ntt(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, const uint64_t *d_plain_ntt, he355_indexer ix, uint64_t *d_out);
int he355_bfv_multiply_plain_accumulate(he355_ctx *ctx, int L, int size, uint64_t rows, uint64_t cols, uint64_t inner, const uint64_t *d_ct, uint64_t ct_stride_i,
                                        uint64_t ct_stride_k, const uint64_t *d_plain_ntt, uint64_t pt_stride_k, uint64_t pt_stride_j, uint64_t *d_out);
/* ---- monomial multiply, oblivious query expansion and ciphertext merge (BFV contexts only, else HE355_E_INVALID_ARGS, decided on the host before any device
 * is asked for; coefficient form; every L in 1..L_top).  he355_bfv_multiply_plain_accumulate scans a database with one ciphertext per
 * index of a dimension -- Enc(1) at the wanted index, Enc(0) elsewhere; instead of encrypting and uploading all of them a client sends
 * ONE ciphertext of sum_k m_k X^k and the server expands it obliviously (Angel, Chen, Laine, Setty, "PIR with compressed queries and
 * amortized query processing", Alg. 3): each level takes one Galois substitution and one multiplication by a monomial.
 *   he355_bfv_multiply_monomial   out = in X^exponent in Z_q_i[X]/(X^N + 1) for every polynomial of [n][size][L][N], size 1..3, exponent in
 *                                 [0, 2N) (X^N = -1); canonical residues: the negative of 0 is 0.  By definition bit-identical to
 *                                 he355_bfv_multiply_plain with the plaintext X^e (coefficient 1) for e < N and with coefficient t - 1 at
 *                                 e - N for e >= N; one streaming launch, no transform.  d_out may not overlap d_in; n == 0 touches nothing.
 *                                 [UPSTREAM-UNVERIFIED] as the level operations above: SEAL's multiply_plain mono path
 *                                 (util::negacyclic_shift_poly_coeffmod).
 *   he355_bfv_expand_galois_elts  the Galois elements he355_bfv_expand needs for `count` children: e_j = N / 2^j + 1, j < d = ceil(log2 count),
 *                                 written to out (at most cap entries); returns d, 0 for a CKKS context or a count outside 1..N.  Their keys
 *                                 come from he355_keygen_galois / he355_set_galois_key (any odd element is accepted there).
 *   he355_bfv_expand              d_in [n][2][L][N], n queries -> d_out [count][n][2][L][N], 1 <= count <= N, CHILD-MAJOR: child k of query r is
 *                                 ciphertext k n + r, the addressing of he355_bfv_multiply_plain_accumulate with ct_stride_i = 1,
 *                                 ct_stride_k = n (transform the children with he355_bfv_transform_to_ntt first).  The definition, every + and -
 *                                 being he355_add / he355_sub on canonical residues: for j = 0 .. d-1, s = 2^j, and every node k < 2^j holding c:
 *                                     g = he355_apply_galois(c, e_j);  child k = c + g;  child k + s = X^(-s) (c - g), only when k + s < count.
 *                                 A query costs 2^d - 1 key switches, one batched key switch per level over the nodes of all queries.  If the
 *                                 query's plaintext is sum_i m_i X^i mod t, child k decrypts to 2^d sum_{i = k mod 2^d} m_i X^(i - k) mod t: for a
 *                                 query supported on i < 2^d the constant 2^d m_k (the client folds 2^-d mod t into the query; t is odd).
 *                                 Refused before the first launch, so that nothing is half-written: a count of 0 or above N, a bad L, a
 *                                 missing Galois key (the message names the element), d_out overlapping d_in.  n == 0 touches nothing;
 *                                 count == 1 copies.  Scratch: one pool block of 2^(d-1) n ciphertexts (a second identical call allocates
 *                                 nothing).  NOT for NTT-form ciphertexts: as in SEAL, transform after the expansion.
 *   he355_bfv_merge               the expansion's transpose: `count` ciphertexts per result become ONE (PackLWEs / the partial-trace merge of
 *                                 Chen, Dai, Kim, Song, "Efficient homomorphic conversion between (ring) LWE ciphertexts", Alg. 2, the response
 *                                 packing of Spiral and Respire), so a server that answers `count` retrievals whose records each fill a
 *                                 1/count share of the ring sends one reply instead of `count`.  Input k < count of result r < n is the
 *                                 ciphertext at index k in_stride_k + r in_stride_r of d_in, strides in ciphertexts of 2 L N words:
 *                                 (n, 1) is what he355_bfv_expand writes, (1, cols) what a scan's [rows][cols] results are; d_out is
 *                                 [n][2][L][N]; 1 <= count <= N, d = ceil(log2 count).  The Galois elements are exactly
 *                                 he355_bfv_expand_galois_elts(count): there is no enumerator of its own, and a client that uploaded expansion
 *                                 keys needs no further key.  The definition, every + and - being he355_add / he355_sub on canonical residues,
 *                                 every X^s he355_bfv_multiply_monomial, slots k >= count absent: for j = d-1 down to 0, s = 2^j, and every
 *                                 slot k < s, with even = slot k and odd = slot k + s:
 *                                     S = even + X^s odd,  D = even - X^s odd      (S = D = even where slot k + s is absent: the first level only)
 *                                     slot k := S + he355_apply_galois(D, e_j)
 *                                 d_out is slot 0 after level 0; count == 1 copies.  The call is bit-identical to this composition of the
 *                                 public calls; it runs one launch and one batched key switch (D, with S as its addend) per level over
 *                                 the pairs of all results, 2^d - 1 key switches per result in all.  If input k decrypts to
 *                                 sum_i mu_(k,i) X^i, the result decrypts to the polynomial whose coefficient k + 2^d m is
 *                                 2^d mu_(k, 2^d m) mod t for k < count and 0 for count <= k < 2^d (the client folds 2^-d mod t in; t is odd):
 *                                 only the coefficients of input k at multiples of 2^d survive, moved up by k, and
 *                                 he355_bfv_merge(he355_bfv_expand(q)) at count = 2^d decrypts to 4^d times the plaintext of q.
 *                                 Refused before the first launch, so that nothing is half-written: a count of 0 or above N, a bad L, strides
 *                                 under which two inputs lie at one place (a stride of 0 along an index that moves, or colliding indices), an
 *                                 extent whose index arithmetic would wrap (past 2^60 words), more pairs than one launch's grid holds, a
 *                                 missing Galois key (the message names the element), d_out overlapping the inputs (d_out may not lie inside
 *                                 their span, a gap between strided inputs included).  n == 0 touches nothing.  Scratch: one pool block of
 *                                 3 2^(d-1) n ciphertexts (2 n at d = 1; a second identical call allocates nothing; if it does not fit, the
 *                                 allocator's error comes before any launch).  Coefficient form only, as the expansion. */
int he355_bfv_multiply_monomial(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_in, uint32_t exponent, uint64_t *d_out);
uint64_t he355_bfv_expand_galois_elts(const he355_ctx *ctx, uint64_t count, uint32_t *out, uint64_t cap);
int he355_bfv_expand(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, uint64_t count, uint64_t *d_out);
int he355_bfv_merge(he355_ctx *ctx, int L, uint64_t n, uint64_t count, const uint64_t *d_in, uint64_t in_stride_k, uint64_t in_stride_r, uint64_t *d_out);
/* ---- ciphertext decomposition for recursive (two-dimensional) PIR (BFV contexts only, coefficient-form ciphertexts, every L in 1..L_top).
 * A database seen as n1 x n2 needs n1 + n2 expanded children instead of n1 n2 (Angel, Chen, Laine, Setty, "Handling larger databases"): scan
 * the first dimension, CUT each of the n2 resulting ciphertexts into plaintexts, scan those with the second dimension's children; the client
 * decrypts, glues the plaintexts back into a ciphertext and decrypts once more.  The cut and its inverse are these calls.
 * [UPSTREAM-UNVERIFIED] as the level operations above; the definition is this library's own:
 *     w = bitlen(t) - 1 (2^w <= t: every w-bit value is a plaintext coefficient), b_i = bitlen(q_i), D_i = ceil(b_i / w),
 *     off_i = sum_{i' < i} D_i', D(L) = off_L, F = size D(L);
 *     digit g < D_i of a canonical residue x under prime i is (x >> (g w)) & (2^w - 1) (every shift below 64);
 *     polynomial k, prime i, digit g of ciphertext r is plaintext r F + k D(L) + off_i + g, coefficient e of it the digit of coefficient e.
 *   he355_bfv_digit_count    returns D(L) and writes D_0 .. D_(L-1) (at most cap entries); 0 for a CKKS context or a bad level.  Host only.
 *   he355_bfv_decompose      d_ct [n][size][L][N] -> d_plain [n][F][N] coefficients mod t, the layout he355_bfv_plain_to_ntt and he355_encrypt
 *                            read; size 1..3; one streaming launch, every ciphertext word read once.
 *   he355_bfv_decompose_ntt  d_ct [n][size][L][N] -> d_plain_ntt [n][F][L_out][N].  By definition bit-identical to he355_bfv_decompose followed
 *                            by he355_bfv_plain_to_ntt(L_out, n F, ..): the centred lift of each digit (below floor((t + 1) / 2) as is, else
 *                            minus t) under primes 0 .. L_out-1, transformed in he355_ntt_forward's bit order.  L and L_out are independent:
 *                            switch the first scan's result down with he355_bfv_mod_switch so that F is small, then scan again at the level
 *                            of the fresh children.  The output is the pt(k, j) operand of he355_bfv_multiply_plain_accumulate as it lies:
 *                            entry k = r, column j = f, pt_stride_k = F, pt_stride_j = 1.  For N >= 2048 the digits are cut and lifted
 *                            inside the forward column pass (neither intermediate slab exists); N = 1024 runs the two calls (one pool block).
 *   he355_bfv_compose        the inverse, d_plain [n][F][N] -> d_ct [n][size][L][N], for the client after he355_decrypt of the second scan:
 *                            residue = sum_g (digit_g masked) 2^(g w), digits below the top one masked to w bits, the top one to
 *                            b_i - (D_i - 1) w bits, so the sum is below 2^b_i < 2 q_i and one conditional subtraction gives a canonical
 *                            residue whatever the input.  On he355_bfv_decompose's own output it is the identity.
 * Refused with HE355_E_INVALID_ARGS on the host, before any device is asked for: a CKKS context, a bad L or L_out, size outside 1..3, t < 2,
 * n F above 2^32 - 1, any overlap of output and input.  n == 0 touches nothing.  Everything is queued on the context's stream. */
uint64_t he355_bfv_digit_count(const he355_ctx *ctx, int L, uint32_t *per_prime, uint64_t cap);
int he355_bfv_decompose(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, uint64_t *d_plain);
int he355_bfv_decompose_ntt(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, int L_out, uint64_t *d_plain_ntt);
int he355_bfv_compose(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_plain, uint64_t *d_ct);
/* ---- the external product RGSW(m) [.] BFV(mu) -> BFV(m mu) (BFV contexts only, every L in 1..L_top).  The later dimensions of a PIR
 * (OnionPIR, Spiral) select with it instead of cutting ciphertexts into plaintexts: its noise grows additively, so the reply stays ONE
 * ciphertext and the client decrypts once.  No special prime is involved.  [UPSTREAM-UNVERIFIED] as the decomposition above; the definition is
 * this library's own:
 *     gadget table at level L: digit_bits = v in 1..63 (the caller's choice: noise against work), b_i = bitlen(q_i), E_i = ceil(b_i / v),
 *     off_i = sum_{i' < i} E_i', E(L) = off_L;
 *     digit g < E_i of a canonical residue x under prime i is (x >> (g v)) & (2^v - 1) as a NON-NEGATIVE integer (no centred lift: d - t equals
 *     d mod t only, and the identity below holds mod q);
 *     gadget element G_(i,g) is 2^(g v) mod q_i under prime i and 0 under every other prime, so for every canonical RNS value
 *     x == sum_(i,g) digit_(i,g)(x_i) G_(i,g) (mod q_L);
 *     polynomial k, prime i, digit g of ciphertext r is digit polynomial r size E(L) + k E(L) + off_i + g (he355_bfv_decompose's order);
 *     an RGSW ciphertext at level L is [2 E(L)][2][L][N] in NTT form, row f = k E(L) + off_i + g: row f of RGSW r is
 *     he355_encrypt_zero(seed, first_index + r 2 E(L) + f) with its polynomials cut to the first L primes (dropping RNS components of an
 *     encryption of zero leaves one), plus lift(m) 2^(g v) mod q_i in polynomial k under prime i only -- lift the centred lift of
 *     he355_bfv_multiply_plain over all N coefficients of m (mod t) -- transformed in he355_ntt_forward's bit order;
 *     rgsw [.] ct = sum_{f < 2 E(L)} NTT_j(digit_f(ct)) (.) row_f(rgsw) per prime j < L and both polynomials, NTT_j(digit_f) the digit
 *     polynomial (the same integers under every prime, reduced mod q_j where v >= b_j) transformed under prime j; the sum is the canonical
 *     residue of the exact integer sum (128-bit unreduced runs, as he355_bfv_multiply_plain_accumulate).
 * If ct has phase Delta mu + e, the result has phase m (Delta mu + e) + sum_f digit_f e_f.
 *   he355_bfv_gadget_count          returns E(L) and writes E_0 .. E_(L-1) (at most cap entries); 0 for a CKKS context, a bad L or a bad v.
 *                                   Host only.
 *   he355_bfv_gadget_decompose      d_ct [n][size][L][N] coefficient form -> d_digits [n][size E][N], coefficient form; size 1..3; one launch.
 *   he355_bfv_gadget_decompose_ntt  -> d_digits_ntt [n][size E][L][N].  By definition bit-identical to he355_bfv_gadget_decompose followed by
 *                                   he355_ntt_forward of every digit polynomial under every prime j < L.  For N >= 2048 a block of the forward
 *                                   column pass reads each ciphertext word once and walks all of its digits and output primes; N = 1024 writes
 *                                   the digits under every prime and transforms in place.  No scratch.
 *   he355_bfv_rgsw_encrypt          d_plain [n][N] mod t -> d_rgsw [n][2E][2][L][N]; needs he355_set_public_key.  At L < L_top the top-level
 *                                   encryptions of zero live in one pool block.
 *   he355_bfv_external_product      d_out(r) = sum_{kappa < inner} rgsw(r, kappa) [.] ct(r, kappa), [n][2][L][N], COEFFICIENT form in and out: it
 *                                   feeds he355_bfv_mod_switch, he355_decrypt or the next external product of a selection tree as it lies.
 *                                   Ciphertext (r, kappa) ([2][L][N]) at index r ct_stride_r + kappa ct_stride_k of d_ct, RGSW (r, kappa) at
 *                                   r rg_stride_r + kappa rg_stride_k of d_rgsw; rg_stride_r == 0: all results share one selector row.  By
 *                                   definition bit-identical to he355_bfv_gadget_decompose_ntt of the inner ciphertexts of each result,
 *                                   he355_bfv_multiply_plain_accumulate(L, 2, 1, 1, inner 2E, ..) per result with the RGSW rows as the ciphertext
 *                                   operand and the digits as the plaintext operand, and he355_bfv_transform_from_ntt.  The digit slab is one
 *                                   pool block, the results split into passes of about 4096 digit polynomials (never fewer than one result).
 * Refused with HE355_E_INVALID_ARGS on the host, before any launch, the output untouched: a CKKS context, L outside 1..L_top, digit_bits
 * outside 1..63, size outside 1..3, inner == 0 or inner 2 E(L) above 2^31 - 1, more polynomials than one launch's grid holds, strides that
 * take an operand past 2^60 words, any overlap of the output with an input (all of these before any device is asked for), and
 * he355_bfv_rgsw_encrypt without a public key.  n == 0 touches nothing.  Everything is queued on the context's stream; a second identical
 * call makes no raw allocation. */
uint64_t he355_bfv_gadget_count(const he355_ctx *ctx, int L, int digit_bits, uint32_t *per_prime, uint64_t cap);
int he355_bfv_gadget_decompose(he355_ctx *ctx, int L, int digit_bits, int size, uint64_t n, const uint64_t *d_ct, uint64_t *d_digits);
int he355_bfv_gadget_decompose_ntt(he355_ctx *ctx, int L, int digit_bits, int size, uint64_t n, const uint64_t *d_ct, uint64_t *d_digits_ntt);
int he355_bfv_rgsw_encrypt(he355_ctx *ctx, int L, int digit_bits, uint64_t n, const uint64_t *d_plain, uint64_t seed, uint64_t first_index, uint64_t *d_rgsw);
int he355_bfv_external_product(he355_ctx *ctx, int L, int digit_bits, uint64_t n, uint64_t inner, const uint64_t *d_ct, uint64_t ct_stride_r, uint64_t ct_stride_k,
                               const uint64_t *d_rgsw, uint64_t rg_stride_r, uint64_t rg_stride_k, uint64_t *d_out);
/* ---- the selection tree: fold `count` ciphertexts with ceil(log2 count) RGSW bits (BFV contexts only, coefficient form in and out, every L in
 * 1..L_top, digit_bits = v in 1..63, E = E(L) as above).  he355_bfv_external_product selects with ONE-HOT selectors, one RGSW ciphertext per
 * candidate; as in OnionPIR and Spiral a selector per BIT of the index folds the candidates pairwise with a CMUX, even + RGSW(b) [.] (odd - even):
 * 32 candidates need 5 selectors, and gadget noise enters m times one after the other instead of as a 2^m-term sum.
 *   he355_bfv_select   leaf k < count of result r < n is the ciphertext [2][L][N] at index r ct_stride_r + k ct_stride_k of d_ct ((cols, 1): a
 *                      scan's [rows][cols] results; (1, n): child-major).  m = ceil(log2 count); selector j < m of result r is the RGSW
 *                      ciphertext [2E][2][L][N] (NTT form) at index r rg_stride_r + j rg_stride_j of d_rgsw ((n_sel, 1): what
 *                      he355_bfv_rgsw_from_bfv writes; rg_stride_r == 0: all results share one set of bits).  d_out is [n][2][L][N].
 *                      The definition, every + and - being he355_add / he355_sub on canonical residues: level j = 0 .. m-1 has c_j nodes per
 *                      result, c_0 = count (the leaves), c_(j+1) = ceil(c_j / 2), and for every p < c_(j+1)
 *                          node'(p) = node(2p) + he355_bfv_external_product(L, v, 1, 1, node(2p+1) - node(2p), RGSW(r, j))   where 2p+1 < c_j,
 *                          node'(p) = node(2p), a copy,                                                                     where 2p+1 = c_j;
 *                      d_out(r) is the one node left after level m-1.  The call is BIT-IDENTICAL to this composition of the public calls.
 *                      count == 1 copies; n == 0 touches nothing.  Meaning: if selector j encrypts the bit b_j and leaf k has phase
 *                      Delta mu_k + e_k, the result decrypts to the leaf with index sum_j b_j 2^j (the least significant bit is consumed
 *                      first) where that index is below count.  Where it is not, the pass-through rule decides: at every level a node
 *                      without a partner is taken whatever the bit says, so the result is the leaf reached by walking down from the root
 *                      and, at level j, going to child 2p + b_j if it exists and to child 2p otherwise (count = 5, bits (1,0,1): leaf 4).
 *                      One level is a pass loop over all pairs of all results: the digits of odd - even are cut straight from the two
 *                      nodes (the difference is never stored), multiplied into the selector's rows, and the inverse column pass adds the
 *                      even node and stores the next level's node; N = 1024 (no column pass) runs he355_ntt_inverse and a streaming add
 *                      instead.  The nodes without a partner are moved by one copy launch per level that has one.
 * Refused with HE355_E_INVALID_ARGS on the host, before any device is asked for, the output untouched: a CKKS context, L outside 1..L_top,
 * digit_bits outside 1..63, count == 0 or above 2^24, leaf strides under which two leaves coincide (a stride of 0 along an index that moves, or
 * colliding indices: he355_bfv_merge's rule), strides that take an operand past 2^60 words, more pairs than one launch's grid holds
 * (n floor(count / 2) 2 L N / 512 above 2^31 - 1, or n above 2^31 - 1), d_out overlapping the leaves' span (a gap between strided leaves
 * included) or the selectors.  The leaves and selectors are only read.  Everything is queued on the context's stream.  Scratch: one pool block
 * of the two alternating node levels, (ceil(count/2) + ceil(count/4)) n ciphertexts (none at m = 1, the first term only at m = 2), and one of the
 * digit slab of a pass of pairs (bfv_gadget_pass over level 0's pairs with 2E terms, about 4096 digit polynomials) with the pass's sums, 2 L
 * polynomials per pair, behind it (N = 1024, whose tail runs once per level: the sums of level 0's n floor(count / 2) pairs); both are taken before the first launch, so the allocator's error comes before any launch, and a second
 * identical call makes no raw allocation. */
int he355_bfv_select(he355_ctx *ctx, int L, int digit_bits, uint64_t n, uint64_t count, const uint64_t *d_ct, uint64_t ct_stride_r, uint64_t ct_stride_k,
                     const uint64_t *d_rgsw, uint64_t rg_stride_r, uint64_t rg_stride_j, uint64_t *d_out);
/* ---- RGSW selectors from ONE packed query ciphertext (BFV contexts only, every L in 1..L_top).  An RGSW ciphertext is [2E][2][L][N] words, and a
 * query of the external-product route carries one per index of a later dimension.  As in OnionPIR and Spiral the client instead packs the
 * selectors' gadget components into coefficients of a query ciphertext, the server expands it with he355_bfv_expand and turns each group of E
 * children into an RGSW ciphertext with one external product by RGSW(s), a key the client sends once.  Notation as above: v the digit width, E_i,
 * off_i, E = E(L), row f = k E + off_i + g, lift the centred lift; a selector is a scalar m in [0, t), the RGSW message the constant polynomial m.
 * [UPSTREAM-UNVERIFIED] as the external product; the definition is this library's own.
 *   he355_bfv_selector_encrypt    (client) d_sel [n][n_sel] mod t -> d_out [n][2][L][N], coefficient form.  With d = ceil(log2 count), the d of
 *                                 he355_bfv_expand(.., count, ..): ciphertext r is he355_encrypt_zero(seed, first_index + r) cut to the first L
 *                                 primes, and for every selector b < n_sel, prime i < L and digit g < E_i the coefficient
 *                                 first_slot + b E + off_i + g of polynomial 0 under prime i ONLY receives
 *                                 lift(m_(r,b)) 2^(g v) (2^d)^(-1) mod q_i; nothing else changes.  After he355_bfv_expand(L, n, .., count, ..) child
 *                                 first_slot + b E + off_i + g has phase lift(m) G_(i,g) plus noise: row (k = 0, i, g) of RGSW(m) before its
 *                                 transform.  No Delta is involved.  first_slot and count let the caller he355_add the result onto an
 *                                 he355_encrypt of the first dimension's one-hot plaintext: first dimension and selectors travel in ONE
 *                                 ciphertext.  Needs he355_set_public_key.  At L < L_top the top-level encryptions of zero live in one pool block.
 *   he355_bfv_rgsw_encrypt_secret (client, once per key) d_rgsw [2 E_key][2][L][N], E_key = E(L) at width key_bits.  By definition bit-identical to
 *                                 he355_bfv_rgsw_encrypt(L, key_bits, 1, d_plain, seed, first_index, ..) with d_plain the secret key's coefficients
 *                                 mod t: 0, 1, and t - 1 for -1.  The context holds s in NTT form (he355_set_secret_key) and brings it to
 *                                 coefficients itself; needs both keys.  Publishing an encryption of s under s is the usual CIRCULAR-SECURITY
 *                                 assumption of these schemes (as for relinearization keys); the library does not weaken or strengthen it.
 *   he355_bfv_rgsw_from_bfv       (server) d_rgsw [n][n_sel][2E][2][L][N], NTT form.  Slot f < E of selector (r, b) is the coefficient-form
 *                                 ciphertext at index r ct_stride_r + (b E + f) ct_stride_k of d_ct; after he355_bfv_expand with nq queries:
 *                                 ct_stride_r = 1, ct_stride_k = nq, d_ct at child first_slot.  By definition bit-identical to: row f (k = 0) of
 *                                 RGSW (r, b) is he355_bfv_transform_to_ntt of the slot-f ciphertext, row E + f (k = 1) is
 *                                 he355_bfv_transform_to_ntt of he355_bfv_external_product(L, key_bits, 1, 1, that ciphertext, .., d_key, 0, 1, ..):
 *                                 RGSW(s) [.] C has phase s phase(C) plus gadget noise, so the k = 1 row carries m G s.  digit_bits (the output's
 *                                 gadget) and key_bits (the conversion's) are independent; a narrow key_bits buys quiet k = 1 rows once per query.
 *                                 Fused: the multiply-accumulate leaves its NTT-form sums in the k = 1 rows as they are (the inverse transform
 *                                 and the transform back are never run), and for N >= 2048 the column pass that cuts the key_bits digits also
 *                                 emits the slot's own column, so the children are read once for both halves.  N = 1024 and calls whose first
 *                                 pass is below he355_bfv_gadget_decompose_ntt's 256-block rule stream instead.  The digit slab is one pool block,
 *                                 split into passes of about 4096 digit polynomials (never less than one slot ciphertext).
 * Refused with HE355_E_INVALID_ARGS on the host, before any launch, the output untouched: a CKKS context, L outside 1..L_top, digit_bits or
 * key_bits outside 1..63, n_sel == 0, count outside 1..N, first_slot + n_sel E > count, strides that take an operand past 2^60 words, more
 * polynomials than one launch's grid holds, any overlap of the output with an input (all of these before any device is asked for), and a
 * missing public or secret key where one is needed (the message says which).  n == 0 touches nothing.  Everything is queued on the context's
 * stream; a second identical call makes no raw allocation. */
int he355_bfv_selector_encrypt(he355_ctx *ctx, int L, int digit_bits, uint64_t n, uint64_t n_sel, uint64_t first_slot, uint64_t count, const uint64_t *d_sel,
                               uint64_t seed, uint64_t first_index, uint64_t *d_out);
int he355_bfv_rgsw_encrypt_secret(he355_ctx *ctx, int L, int key_bits, uint64_t seed, uint64_t first_index, uint64_t *d_rgsw);
int he355_bfv_rgsw_from_bfv(he355_ctx *ctx, int L, int digit_bits, int key_bits, uint64_t n, uint64_t n_sel, const uint64_t *d_ct, uint64_t ct_stride_r,
                            uint64_t ct_stride_k, const uint64_t *d_key, uint64_t *d_rgsw);
/* ---- a PIR database from packed bytes (BFV contexts only).  The scan, the expansion and the cut above take the database as an [n][L][N]
 * slab of NTT-form plaintexts; what a user holds is bytes.  These calls are the device path between the two, and the client's way back
 * after he355_decrypt.  [UPSTREAM-UNVERIFIED] as the decomposition; the definition is this library's own:
 *     w = bitlen(t) - 1, the digit width of he355_bfv_decompose (2^w <= t: every w-bit value is a plaintext coefficient);
 *     a plaintext holds B bytes, 1 <= B <= Bmax = floor(N w / 8); the bytes of plaintext j are buf[j stride, j stride + B), read as ONE
 *     little-endian integer v_j; coefficient e < N of plaintext j is (v_j >> (e w)) & (2^w - 1), which is 0 once e w >= 8 B; the last non-zero
 *     field is zero-extended and never borrows from bytes at or beyond j stride + B;
 *     the inverse masks every coefficient to w bits, ORs it in at bit e w and keeps the low 8 B bits.
 * How records are laid into the B bytes (whole records per plaintext, padding up to stride) is the caller's business.
 *   he355_bfv_bytes_per_plain   returns Bmax and writes w (field_bits may be null); 0 for a CKKS context.  Host only.
 *   he355_bfv_unpack_bytes      d_bytes -> d_plain [n][N] coefficients mod t, the layout he355_encrypt and he355_bfv_plain_to_ntt read.
 *                               d_bytes may be ANY byte address inside a device allocation and stride_bytes any value >= bytes_per_plain: a
 *                               contiguous byte array with stride = B is a database as it lies.  The kernel reads only aligned 8-byte words
 *                               that contain at least one valid byte of the plaintext it is working on.  d_plain must be 16-byte
 *                               aligned (a lane stores two coefficients at once).
 *   he355_bfv_unpack_bytes_ntt  d_bytes -> d_plain_ntt [n][L_out][N].  By definition bit-identical to he355_bfv_unpack_bytes followed by
 *                               he355_bfv_plain_to_ntt(L_out, n, ..); the output is the pt(k, j) operand of
 *                               he355_bfv_multiply_plain_accumulate.  For N >= 2048 the fields are cut and lifted inside the forward column
 *                               pass (neither the coefficient slab nor the lifted slab exists); N = 1024 runs the two calls, 4096
 *                               plaintexts at a time through one pool block.
 *   he355_bfv_pack_bytes        the inverse, d_plain [n][N] -> d_bytes, for the client after he355_decrypt.  It writes whole words,
 *                               ceil(B / 8) per plaintext, the bytes past B in the last word zero; nothing else inside stride is touched.
 *                               d_bytes must be 8-byte aligned, stride_bytes a multiple of 8 and at least 8 ceil(B / 8) (two plaintexts never
 *                               share a word).  The input may be any 64-bit words: each is masked to w bits.
 * Refused with HE355_E_INVALID_ARGS on the host, before any device is asked for, the output untouched: a CKKS context, L_out outside
 * 1..L_top, B == 0 or B > Bmax, stride < B, (n - 1) stride + B at or above 2^63 (a checked multiply: no address can wrap), a d_plain of
 * he355_bfv_unpack_bytes that is not 16-byte aligned, pack's alignment rules, n N / 256 above 2^31 - 1 (one launch's grid), any overlap
 * of output and input.  n == 0 touches nothing.  Everything is queued on the context's stream. */
uint64_t he355_bfv_bytes_per_plain(const he355_ctx *ctx, uint32_t *field_bits);
int he355_bfv_unpack_bytes(he355_ctx *ctx, uint64_t n, const void *d_bytes, uint64_t stride_bytes, uint64_t bytes_per_plain, uint64_t *d_plain);
int he355_bfv_unpack_bytes_ntt(he355_ctx *ctx, int L_out, uint64_t n, const void *d_bytes, uint64_t stride_bytes, uint64_t bytes_per_plain, uint64_t *d_plain_ntt);
int he355_bfv_pack_bytes(he355_ctx *ctx, uint64_t n, const uint64_t *d_plain, uint64_t bytes_per_plain, uint64_t stride_bytes, void *d_bytes);
/* ---- reply compression (BFV contexts only).  The last server step of a PIR round trip is he355_bfv_mod_switch to L = 1: two polynomials of
 * 64-bit words under q = q_0, the first prime of the chain.  These calls switch the two halves of such a reply to the moduli 2^k0 (c0) and
 * 2^k1 (c1), pack the bits, and decrypt the packed reply on the client.  [UPSTREAM-UNVERIFIED] the idea is SealPIR's, OnionPIR's and
 * Spiral's; the definition is this library's own, exact integers, no tolerance:
 *     switch     : for x in [0, q): cut_k(x) = floor((x 2^k + floor(q / 2)) / q) mod 2^k (q is odd: no ties; an x that rounds to 2^k wraps to 0);
 *     layout     : one reply is the little-endian bit string of c0's N fields of k0 bits, then c1's N fields of k1 bits, coefficient e at bit
 *                  e k.  N >= 1024, so c1 starts on a word boundary and a reply is exactly N (k0 + k1) / 64 whole 64-bit words,
 *                  N (k0 + k1) / 8 bytes; fields straddle words whenever k does not divide 64;
 *     decryption : unpack y0, y1; y1 centred is y1 - 2^k1 where y1 >= 2^(k1 - 1); w is the centred representative mod q_0 of its negacyclic
 *                  product with the secret key (the integer product whenever N 2^(k1 - 1) |s|_inf < q_0 / 2: every accepted k1, ternary
 *                  keys); z = (y0 2^(k1 - k0) + w) mod 2^k1; M = floor((t z + 2^(k1 - 1)) / 2^k1); the plaintext coefficient is M mod t;
 *                  per reply r = the largest |t z - M 2^k1|, noise_bits = bit length of r, budget = max(0, k1 - noise_bits - 1):
 *                  he355_bfv_noise_budget's formula with 2^k1 in the place of q;
 *     accepted   : 2 <= k0 <= k1 and N 2^(k1 - 1) <= (q_0 - 1) / 2 (a 60-bit q_0: k1 <= 46 at N = 8192, k1 <= 44 at N = 32768);
 *     safe       : k0 = bitlen(t) + 2, k1 = bitlen(t) + 2 + log2 N: for a ternary key and an input with at least 2 bits of invariant noise
 *                  budget at L = 1 every coefficient decrypts correctly (|v'| <= 2^-3 + t 2^-(k0+1) + t N 2^-(k1+1) < 3/8); the reported
 *                  budget may still be 0 there (the clamp).  Tighter widths are the caller's risk; the budget output says what is left.
 *   he355_bfv_reply_bytes      bytes per reply, or 0 for a CKKS context or refused widths.  Host only.
 *   he355_bfv_reply_safe_bits  writes the safe widths; returns 1 if they are accepted on this chain, else 0 (a 35-bit q_0 cannot hold
 *                              them; 0 and nothing written for a CKKS context).  Host only.
 *   he355_bfv_reply_compress   d_ct [n][2][L][N] coefficient form -> reply j at d_bytes + j stride_bytes.  For L > 1 it is, by definition,
 *                              bit-identical to he355_bfv_mod_switch(L -> 1) followed by the L = 1 call (the L = 1 ciphertexts pass through
 *                              one pool block).  d_bytes 8-byte aligned, stride_bytes a multiple of 8 and at least the reply size; nothing
 *                              outside a reply's own words is written.
 *   he355_bfv_reply_decrypt    replies -> d_plain [n][N] coefficients mod t, the layout he355_decrypt writes (it feeds he355_bfv_pack_bytes
 *                              and he355_bfv_decode); d_budget, d_noise_bits int32 [n] on the device, either may be NULL.  Needs
 *                              he355_set_secret_key and nothing else: one transform less per reply than he355_decrypt.
 * Refused with HE355_E_INVALID_ARGS on the host, before any device is asked for, the outputs untouched: a CKKS context, L outside 1..L_top,
 * widths outside the rule above, a d_bytes that is not 8-byte aligned, a stride that is too small or not a multiple of 8,
 * (n - 1) stride + the reply size at or above 2^63 (a checked multiply), a grid above 2^31 - 1 blocks (n N / 256, or n times the 256-word
 * blocks of a reply), any overlap of output and input; and, before the first launch, a missing secret key for the decrypt.  n == 0 touches nothing.  Everything is queued on
 * the context's stream. */
uint64_t he355_bfv_reply_bytes(const he355_ctx *ctx, int k0, int k1);
int he355_bfv_reply_safe_bits(const he355_ctx *ctx, int *k0, int *k1);
int he355_bfv_reply_compress(he355_ctx *ctx, int L, int k0, int k1, uint64_t n, const uint64_t *d_ct, void *d_bytes, uint64_t stride_bytes);
int he355_bfv_reply_decrypt(he355_ctx *ctx, int k0, int k1, uint64_t n, const void *d_bytes, uint64_t stride_bytes, uint64_t *d_plain, int32_t *d_budget,
                            int32_t *d_noise_bits);
/* ---- seeded BFV queries and Galois keys (BFV contexts only).  A secret-key encryption (c0, c1) has a uniform c1: the client sends c0 and the
 * SEED of c1, and the server regenerates c1 on the device.  That halves every query ciphertext and every Galois key on the way up.
 * [UPSTREAM-UNVERIFIED] the idea is SEAL's encrypt_zero_symmetric with a seeded c1 (Serializable<>), SealPIR's, OnionPIR's and Spiral's;
 * the definition is this library's own, exact integers, no tolerance:
 *     seeds      : a_seed IS PUBLIC AND TRAVELS WITH THE CIPHERTEXT.  noise_seed IS SECRET AND NEVER LEAVES THE CLIENT.  THE TWO MUST
 *                  DIFFER: the generator is the library's counter-based one (csrc/client/sampler.h), whose mixing step splitmix64 is
 *                  invertible, so whoever knows the seed of a stream knows the stream -- a call with a_seed == noise_seed would publish
 *                  the error and is refused.  THE GENERATOR IS NOT A CRYPTOGRAPHIC XOF: the seeded half is only as unpredictable as
 *                  splitmix64 makes it, exactly like every other random polynomial of this library; swapping in an XOF (SHAKE, BLAKE2
 *                  as SEAL does) is out of scope here.  A (a_seed, index) pair must never be reused for two different ciphertexts, and a
 *                  noise_seed never with another a_seed.
 *     streams    : ciphertext r of a call is seeded ciphertext first_index + r, below 2^40.  Its uniform half under prime i uses stream
 *                  seeded_a_stream(first_index + r, i) = 2^48 + 64 (first_index + r) + i, its error stream
 *                  seeded_e_stream(first_index + r) = 2^48 + 64 (first_index + r) + 63 (sampler.h): apart from enc_stream and keygen_stream.
 *     seeded half: IN NTT FORM, the form he355_keygen_* sample in: a^_i[n] = sample_uniform_at(a_seed, seeded_a_stream(first_index + r, i), n, q_i),
 *                  n the position in he355_ntt_forward's output order.
 *     seeded zero: at level L, built there (no special prime, no divide-and-round): c0_i = (-e - iNTT_i(a^_i (.) s^_i)) mod q_i with
 *                  e[n] = sample_cbd_at(noise_seed, seeded_e_stream(first_index + r), n), and c1_i = iNTT_i(a^_i).  (c0, c1) is an ordinary
 *                  coefficient-form BFV ciphertext [2][L][N] with phase c0 + c1 s = -e: every existing call accepts it.
 *   he355_bfv_seeded_encrypt          (client) d_plain [n][N] mod t, or NULL for zeros -> d_c0 [n][L][N], coefficient form.  By definition d_c0
 *                                     followed by he355_bfv_seeded_restore(ntt_form 0) is bit-identical to he355_bfv_add_plain(L, 2, ..) applied
 *                                     to the restored seeded zero.  Needs he355_set_secret_key and nothing else.
 *   he355_bfv_seeded_selector_encrypt (client) polynomial 0 of he355_bfv_selector_encrypt with its public-key zero replaced by the seeded zero:
 *                                     the same plants in the same places, d_c0 [n][L][N].  The first dimension joins as before: the caller adds
 *                                     this c0 to the he355_bfv_seeded_encrypt c0 of ANOTHER index range with he355_add(L, 1, n, ..) and sends
 *                                     the one sum with both first_index values; the server restores the sum under one range and a zero c0 under
 *                                     the other (or both c0's, if they travel apart) and adds the two with he355_add(L, 2, n, ..) -- the sum is a
 *                                     ciphertext of the sum under the sum of the two seeded halves.
 *   he355_bfv_seeded_restore          (server) d_c0 [n][L][N] -> d_out [n][2][L][N].  ntt_form 0: c0 copied, c1 = iNTT(a^): what he355_bfv_expand
 *                                     reads.  ntt_form 1: c0 = NTT(c0), c1 = a^: the rows the NTT-form calls read, bit-identical to
 *                                     he355_bfv_transform_to_ntt of the other form.  Needs no key and no scratch.
 *   he355_keygen_galois_seeded        (client) the `b` halves [L_top][K][N], NTT form, of the Galois key of galois_elt into a DEVICE buffer; digit j,
 *                                     prime i: a = sample_uniform_at(a_seed, keygen_stream(2 + elt, j, K, i), n, q_i), e = sample_cbd_at(noise_seed,
 *                                     keygen_stream(2 + elt, j, K, K), n), b = -(a s + NTT(e)) + [i == j] (P mod q_j) s(X^elt) -- he355_keygen_galois's
 *                                     key with the one seed split in two.  Installs nothing.  One a_seed may serve every element of a client.
 *   he355_set_galois_key_seeded       (server) h_b [L_top][K][N] on the HOST -> key[j][0]; key[j][1] generated on the device from a_seed; by
 *                                     definition bit-identical to he355_set_galois_key of the full key [L_top][2][K][N].
 * Refused with HE355_E_INVALID_ARGS on the host, before any device is asked for, the outputs untouched: a CKKS context, L outside 1..L_top,
 * ntt_form outside {0, 1}, a_seed == noise_seed, first_index + n wrapping or above 2^40, a slab of more than 2^60 words, a grid above
 * 2^31 - 1 blocks (n L N / 512; restore: 2 n L N / 512), any overlap of output and input, he355_bfv_selector_encrypt's own rules, an invalid
 * Galois element, a chain without a special prime; and, before the first launch, a missing secret key (the three client calls).  n == 0
 * touches nothing.  Everything is queued on the context's stream; he355_set_galois_key_seeded returns with the key installed. */
int he355_bfv_seeded_encrypt(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain, uint64_t a_seed, uint64_t noise_seed, uint64_t first_index, uint64_t *d_c0);
int he355_bfv_seeded_selector_encrypt(he355_ctx *ctx, int L, int digit_bits, uint64_t n, uint64_t n_sel, uint64_t first_slot, uint64_t count, const uint64_t *d_sel,
                                      uint64_t a_seed, uint64_t noise_seed, uint64_t first_index, uint64_t *d_c0);
int he355_bfv_seeded_restore(he355_ctx *ctx, int L, int ntt_form, uint64_t n, const uint64_t *d_c0, uint64_t a_seed, uint64_t first_index, uint64_t *d_out);
int he355_keygen_galois_seeded(he355_ctx *ctx, uint32_t galois_elt, uint64_t a_seed, uint64_t noise_seed, uint64_t *d_b);
int he355_set_galois_key_seeded(he355_ctx *ctx, uint32_t galois_elt, const uint64_t *h_b, uint64_t a_seed);
/* Decryptor::invariant_noise_budget, batched: how many bits of noise budget each ciphertext has left AT ITS LEVEL -- what a caller asks
 * before he355_bfv_mod_switch ("is the switch safe?") or another multiply.  BFV contexts only; needs he355_set_secret_key.
 * d_ct [n][size][L][N] coefficient form, size 2 or 3, 1 <= L <= L_top (<= 16, as he355_decrypt).
 * d_budget [n] int32 (device): max(0, bits(q_L) - noise_bits - 1)
 * d_noise_bits [n] int32 (device) or NULL: significant bits of the norm below, BEFORE the clamp.
 * Per ciphertext, q_L the product of the first L primes: phase = c0 + c1 s (+ c2 s^2) per prime (coefficient form), every residue times
 * t mod q_i, CRT-composed to x in [0, q_L), |x| = q_L - x where x >= (q_L + 1) / 2 else x, norm = the largest |x| over the N coefficients,
 * noise_bits = bit length of norm (0 for 0).  Exact integers: no tolerance.  Queued on the context's stream like he355_decrypt (no
 * he355_sync needed after an asynchronous producer; outputs valid after he355_sync / he355_download).  n == 0 touches nothing.
 * [UPSTREAM-UNVERIFIED] as the level operations above: SEAL v3.7.2 decryptor.cpp, invariant_noise_budget. */
int he355_bfv_noise_budget(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, int32_t *d_budget, int32_t *d_noise_bits);
/* out = in[0] + ... + in[n-1] (one ciphertext): the add_inplace accumulation of collapseCKKS, src/engine/seal_context.cpp:401 */
int he355_sum(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_in, uint64_t *d_out);
/* CKKS: out(i,j) = sum_k multiply(a(i,k), b(k,j)), size-3 results [rows*cols][3][L][N]; ciphertext (i,k) of a is at index
 * i*a_stride_i + k*a_stride_k, (k,j) of b at k*b_stride_k + j*b_stride_j — the multiply/add_inplace loop of
 * src/benchmarks/ckks/seal_ckks_matmult_cipherbatchaxis_benchmark.cpp:404-420 */
int he355_multiply_accumulate(he355_ctx *ctx, int L, uint64_t rows, uint64_t cols, uint64_t inner, const uint64_t *d_a, uint64_t a_stride_i,
                              uint64_t a_stride_k, const uint64_t *d_b, uint64_t b_stride_k, uint64_t b_stride_j, uint64_t *d_out);
/* BFV: out(i,j) = sum_k relinearize(multiply(a(i,k), b(k,j))), size-2 results [rows*cols][2][L][N], same addressing -- the
 * multiply / relinearize_inplace / add_inplace loop of src/benchmarks/bfv/seal_bfv_matmult_cipherbatchaxis_benchmark.cpp:398-410 with
 * the inner index inside the batch; d_out may not overlap an operand */
int he355_bfv_multiply_relin_accumulate(he355_ctx *ctx, int L, uint64_t rows, uint64_t cols, uint64_t inner, const uint64_t *d_a, uint64_t a_stride_i,
                                        uint64_t a_stride_k, const uint64_t *d_b, uint64_t b_stride_k, uint64_t b_stride_j, uint64_t *d_out);
/* relinearize_inplace + rescale_to_next_inplace of size-3 ciphertexts (same file :436-437): [n][3][L][N] -> [n][2][L-1][N] */
int he355_relinearize_rescale(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_ct3, uint64_t *d_out);
int he355_rescale(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_in, uint64_t *d_out);         /* -> [n][size][L-1][N] */
int he355_apply_galois(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, uint32_t galois_elt, uint64_t *d_out);
int he355_rotate(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, int step, uint64_t *d_out);
/* d_out[i] = rotate(d_in[i], h_steps[i]), i < n: the rotate_vector(dot_i, -i) loop of collapseCKKS (src/engine/seal_context.cpp:389-392)
 * as batched key switches (ciphertexts that need the same Galois element at the same point of their NAF sequence go together).
 * h_steps: host array of n steps.  Not in place. */
int he355_rotate_each(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, const int32_t *h_steps, uint64_t *d_out);
/* d_out = d_addend + rotate(d_in, step): the rotate + add_inplace pair of the row-major MatMult inner loop
 * (src/benchmarks/bfv/seal_bfv_matmult_row_benchmark.cpp:525-531) and of accumulateCKKS/BFV (src/engine/seal_context.cpp:337-338,
 * 302-303) as one pipeline.  d_addend may be d_out (add in place) when the step has its own Galois key; d_in may be neither. */
int he355_rotate_add(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, int step, const uint64_t *d_addend, uint64_t *d_out);
/* d_out = d_in + sum_j rotate(d_in, h_steps[j]), j < n_steps: the whole inner loop of the row-major MatMult
 * (src/benchmarks/bfv/seal_bfv_matmult_row_benchmark.cpp:519-531, src/benchmarks/ckks/seal_ckks_matmult_row_benchmark.cpp:502-514).  Each rotation
 * is Evaluator::rotate_internal's (own Galois key, else NAF terms least significant first); rotations whose term sequences share a
 * prefix share that prefix's ciphertext, which is computed once -- bit-identical to the unshared loop.  *key_switches (optional):
 * Galois key switches issued per ciphertext.  h_steps: host array.  Not in place. */
int he355_rotate_sum(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, const int32_t *h_steps, uint64_t n_steps, uint64_t *d_out,
                     uint64_t *key_switches);
/* Hoisted rotations (Halevi-Shoup): ONE ciphertext batch under MANY Galois elements, the digit lift of c1 -- everything of a key switch in
 * front of the key product -- run once and shared by all of them (the diagonal method, baby-step/giant-step transforms, the slot <->
 * coefficient maps, convolutions).  The definition is the library's own and NOT bit-identical to he355_apply_galois: for (c0, c1) at
 * level L, element g with installed key key_g and g^-1 its inverse mod 2N,
 *   key' = every residue polynomial of key_g permuted in NTT form by g^-1;  (u0, u1) = the ordinary key switch of c1 under key' added into
 *   (c0, 0);  out = sigma_g applied to both polynomials (the NTT-domain permutation, or the signed coefficient gather for coefficient form)
 * -- the digits of sigma(c1) are non-negative residues of -x where sigma of the digits is -(residue of x); they differ by multiples of q_j
 * that the key absorbs, so the result decrypts to the same rotation with noise of the same bound.  g = 1 is the identity (out = in, no key).
 * key' is built on first use and kept per element until that element's key is installed again or he355_hoist_release_keys: it DOUBLES the
 * device memory of every hoisted element's key.  All chunks of a call run on one stream.  Every refusal is made on the host before any
 * device work; n == 0 or n_elts == 0 touches nothing and returns success.  d_out may overlap neither d_in nor d_plain.
 *
 * out[r][i] = hoisted Galois map of in[i] under h_elts[r]; d_out [n_elts][n][2][L][N] (element-major).
 * ntt_form: CKKS contexts 1 only; BFV contexts 0 = coefficient form (BFV kernels), 1 = NTT-form BFV ciphertexts (NTT-domain pipeline). */
int he355_apply_galois_hoisted(he355_ctx *ctx, int L, int ntt_form, uint64_t n, const uint64_t *d_in, const uint32_t *h_elts, uint64_t n_elts,
                               uint64_t *d_out);
/* the same by steps (step 0 = identity); every non-zero step needs its OWN Galois key: no NAF fallback, a chain cannot be hoisted */
int he355_rotate_hoisted(he355_ctx *ctx, int L, int ntt_form, uint64_t n, const uint64_t *d_in, const int32_t *h_steps, uint64_t n_steps,
                         uint64_t *d_out);
/* out[i] = sum_r plain[r] (.) hoisted(in[i], step r): the diagonal method's inner loop.  NTT-form ciphertexts only (CKKS; BFV as from
 * he355_bfv_transform_to_ntt), d_plain [n_steps][L][N] NTT-form plaintexts shared by the batch, d_out [n][2][L][N]; no rescale.  Equal bit
 * for bit to he355_multiply_plain + he355_add over the hoisted terms (canonical residues; modular addition is exact). */
int he355_rotate_hoisted_plain_sum(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, const int32_t *h_steps, uint64_t n_steps,
                                   const uint64_t *d_plain, uint64_t *d_out);
/* The same sum with ONE mod-down ("double hoisting"): the key products stay in the extended basis Q P, are permuted, multiplied by plaintexts
 * that also carry a residue under the special prime P = q_{K-1} and accumulated there; the part that needs no key is accumulated in Q.
 * d_plain_qp [n_steps][L + 1][N], NTT form: rows 0 .. L - 1 under the data primes, row L under P (he355_plain_extend_special makes it).
 *   d^_{j,i}   = the digits he355_apply_galois_hoisted lifts: c1[j] if i == j, else NTT_i(iNTT_j(c1[j]) mod q_i), i over the L data primes and P
 *   S_r[k][i]  = sum_j d^_{j,i} (.) key'_r[j][k][i]                                   (keyed r; key'_r as above; no mod-down)
 *   A[k][i]    = sum_{r keyed} sigma_{g_r}(S_r[k][i]) (.) plain_qp[r][i]              (L + 1 primes)
 *   B[0][i]    = sum_{r keyed} sigma_{g_r}(c0[i]) (.) plain_qp[r][i] + sum_{r identity} c0[i] (.) plain_qp[r][i];  B[1][i] = sum_{r identity} c1[i] (.) plain_qp[r][i]
 *   out[k][i]  = B[k][i] + (A[k][i] - NTT_i(delta_i)) P^-1 mod q_i,  h = floor(P / 2),  rho = (iNTT_P(A[k][L]) + h) mod P,
 *                delta_i = (rho mod q_i - h mod q_i) mod q_i                           (a sum with no keyed element is B alone)
 * Not the bits of he355_rotate_hoisted_plain_sum (a sum of mod-downs; this is the mod-down of a sum): the same plaintext after decryption,
 * noise no larger, one rounding instead of n_steps.  The step rules, refusals and memory of the permuted keys are that call's. */
int he355_rotate_hoisted_plain_sum_lazy(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, const int32_t *h_steps, uint64_t n_steps,
                                        const uint64_t *d_plain_qp, uint64_t *d_out);
/* d_plain_ntt [n][L][N] NTT-form plaintexts -> d_plain_qp [n][L + 1][N]: rows 0 .. L - 1 copied, row L = NTT_P(c mod P) with c the
 * coefficients under prime 0 centred into (-q_0 / 2, q_0 / 2].  Exact when the plaintext's integer coefficients lie in that range: always
 * for he355_bfv_plain_to_ntt's, for a CKKS plaintext when its scale leaves a bit of q_0.  d_mismatch (optional, one device word): the number
 * of (coefficient, prime i >= 1) pairs whose residue is not c mod q_i -- 0: every prime agrees with prime 0; always 0 when L = 1; null skips
 * the check and its transforms.  Needs a special prime (K >= 2); the two slabs may not overlap; n == 0 touches nothing. */
int he355_plain_extend_special(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain_ntt, uint64_t *d_plain_qp, uint64_t *d_mismatch);
/* The baby-step/giant-step linear transform on the hoisted rotations: for R = n_baby * n_giant diagonals about n_baby + n_giant key products
 * and Galois keys instead of R - 1.
 *   out[c] = sum_j rot_{G_j}( sum_i plain[j][i] (.) rot_{b_i}(in[c]) ),   b = h_baby, G = h_giant (steps; 0 = the identity)
 * NTT-form ciphertexts only (CKKS; BFV as from he355_bfv_transform_to_ntt), d_in and d_out [n][2][L][N], no rescale.  d_plain_qp
 * [n_giant][n_baby][L + 1][N] in the layout of he355_plain_extend_special, shared by the batch.  The caller supplies the plaintexts already
 * PRE-ROTATED, plain[j][i] = rot_{-G_j}(diag_{G_j + b_i}): rot_G(p (.) x) = rot_G(p) (.) rot_G(x), so the outer rotation turns them back into
 * the diagonals.  h_mask [n_giant][n_baby] bytes, may be null (every term): a zero byte means the term is absent.  A step is USED when a
 * term that is not masked names it; every used non-zero step needs its OWN Galois key (no NAF fallback), a step that is not used needs none.
 * The definition (all residues canonical; i over the L data primes and P, tile L = P; sigma_g the NTT-domain permutation; key'_g, the
 * digits and the key product S without a mod-down as for he355_rotate_hoisted_plain_sum_lazy; mod_down that call's last line with B = 0):
 *   1. baby terms, per ciphertext (the digits of c1 lifted once):
 *        keyed i, element g:  T_i[k][i'] = sigma_g(S_i[k][i']),  and  T_i[0][i'] += P sigma_g(c0[i'])  on the data primes
 *        identity:            T_i = (P c0, P c1) on the data primes, 0 under P
 *   2. inner sum, per used row j:  E_j[k][i'] = sum_{i used} T_i[k][i'] (.) plain[j][i][i']            (L + 1 primes)
 *   3. giant step:  identity row: Acc += E_j in Q P (no mod-down);
 *                   keyed row, element h: e_j = mod_down(E_j) (a size-2 ciphertext in Q); S'_j = the key product of the digits of e_j[1]
 *                   under key'_h;  Acc[k] += sigma_h(S'_j[k]),  Acc[0] += P sigma_h(e_j[0]) on the data primes
 *   4. out = mod_down(Acc)
 * Two exact facts let an implementation choose its buffers without changing a bit: mod_down(A + P B) = B + mod_down(A), because rho depends
 * on the P-residue alone -- so c0 may be folded in as P c0 (here) or kept in a Q-side accumulator (the lazy call); and mod_down(P X) = X
 * (rho = h, delta = 0), so a mod-down whose input has no key product in it may be skipped or run: the bits are the same.
 * Refused on the host before any device work; n == 0, n_baby == 0 or n_giant == 0 touches nothing and returns success.  d_out may overlap
 * neither d_in nor any word of d_plain_qp.  The call takes its baby store and two Q P blocks from the context's pool before its first
 * launch (the allocator's error if they do not fit); he355_linear_transform_bsgs_scratch_bytes is an upper bound of that at the context's
 * batch chunk: (n_baby + 2) blocks of min(chunk, n) [2][L + 1][N] ciphertexts, each rounded up by a size class of the pool; saturated at
 * 2^64 - 1; 0 for a level out of range, for nothing to do and for more than 2^20 baby steps (the call refuses them).  The table of used
 * terms lies in the context's own table ring, which is never rewritten under a queued launch: calls may follow each other without a sync. */
int he355_linear_transform_bsgs(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in, const int32_t *h_baby, uint64_t n_baby, const int32_t *h_giant,
                                uint64_t n_giant, const uint64_t *d_plain_qp, const uint8_t *h_mask, uint64_t *d_out);
uint64_t he355_linear_transform_bsgs_scratch_bytes(const he355_ctx *ctx, int L, uint64_t n, uint64_t n_baby);
/* What the hoisted calls of this context did since he355_device_init (or the last call with reset != 0); they count in no field of
 * he355_path_stats_t. */
typedef struct he355_hoist_stats {
    uint64_t digit_lifts;   /* digit-lift sequences: one per chunk with a non-identity element, however many elements          */
    uint64_t key_products;  /* key-product + mod-down + finish sequences: one per (chunk, non-identity element)                 */
    uint64_t keys_permuted; /* permuted key copies built (first use, and again after the element's key was installed again)     */
    uint64_t key_bytes;     /* device bytes the permuted copies hold now (a level: kept across reset)                            */
    uint64_t mod_downs;     /* mod-downs: one per key product for the eager calls, one per chunk with a non-identity element for
                             * he355_rotate_hoisted_plain_sum_lazy, one per (chunk, used keyed giant row) and one per chunk for
                             * he355_linear_transform_bsgs (its digit_lifts: one per chunk with a used keyed baby and one per used
                             * keyed giant row; its key_products: used keyed babies + used keyed giant rows, per chunk)             */
    uint64_t inner_sums;    /* he355_linear_transform_bsgs: inner sums, one per (chunk, used giant row)                               */
    uint64_t reserved[2];
} he355_hoist_stats_t;
int he355_hoist_stats(he355_ctx *ctx, he355_hoist_stats_t *out, int reset);
int he355_hoist_release_keys(he355_ctx *ctx);   /* frees the permuted copies; they are rebuilt on next use */
/* ---- polynomial evaluation (CKKS) on a fused scalar combination ----
 * he355_combine_scalars: out = sum_t a_t * ct_t + a_const, a constant polynomial being the same residue in every NTT slot:
 *   out[c][k][i][e] = (sum_t h_scalars[t][i] * term_t[c][k][i][e] + (k == 0 ? h_const[i] : 0)) mod q_i,   i < L
 * Everything canonical in and out; the integer sum is reduced once.  Term t is [n][size][L_t][N] with L_t = h_terms[t].L >= L, read with
 * its own stride: rows >= L are ignored (he355_mod_switch_drop's rule, no copy).  Terms may repeat a pointer.  Residues are added whatever
 * they stand for, as he355_add: any context (CKKS, NTT-form BFV).  One streaming launch (k_scalar_combine): T reads and one write.
 * Refused on the host before any device work (HE355_E_INVALID_ARGS, the message names the call): L outside 1..L_top, a term level below L
 * or above L_top, size outside 2..3, null lists or null terms with work to do, more than 2^20 terms, a scalar or constant >= q_i, slabs
 * past 2^60 words or wrapping the address space, d_out overlapping any word of any term, n_terms == 0 with a constant.  n == 0, or
 * n_terms == 0 without a constant, touches nothing and succeeds.  The term table lies in the context's table ring: calls may follow
 * each other without a sync. */
typedef struct { const uint64_t *d_ct; int32_t L; int32_t reserved; } he355_term; /* [n][size][L][N], L >= the call's L */
int he355_combine_scalars(he355_ctx *ctx, int L, int size, uint64_t n, const he355_term *h_terms, uint64_t n_terms,
                          const uint64_t *h_scalars /* [n_terms][L] canonical residues */, const uint64_t *h_const /* [L] or NULL */,
                          uint64_t *d_out /* [n][size][L][N] */);
/* Host only: out[i] = a mod q_i for i < L, a = the integer nearest v, ties to even (Python: int(round(v)) % q_i); a negative a gives
 * q_i - (|a| mod q_i), or 0.  A double >= 2^52 is its own integer, taken exactly as m * 2^e in 128 bits.  Refused: non-finite v,
 * |v| >= 2^126, L outside 1..L_top, null out. */
int he355_ckks_scalar_residues(const he355_ctx *ctx, int L, double v, uint64_t *out /* [L] */);
/* he355_ckks_eval_poly: out = p(in), p(x) = sum_k c_k x^k (monomial basis, real coefficients, trailing zeros trimmed), on a power tree
 * of logarithmic depth.  d_in [n][2][L][N] at scale in_scale -> d_out [n][2][L - depth][N] at the nominal scale out_scale.
 * The definition (tests/ckks_eval_poly_ref.py restates it on the oracle).  "Level" is the number of data primes; q[l] is prime index l,
 * the one a rescale from l + 1 primes drops.  All scale arithmetic is IEEE double in the order written.
 *   powers  m = 2^log_baby; babies x^1 .. x^(m-1), giants x^(m 2^j) while the exponent is <= the degree.  A power is computed only if a
 *           non-zero coefficient's leaf uses it, a node's split uses it, or a needed power is built from it.
 *           x^k = x^floor(k/2) * x^ceil(k/2): the higher operand dropped to the lower one's level l, one he355_multiply_relin with rescale:
 *           level l - 1, scale s_a * s_b / q[l - 1].  (x^k lies at level L - ceil(log2 k).)
 *   eval(p, Lt, S), deg p < m (a leaf):  T = S * q[Lt]; per non-zero c_k, k >= 1, the scalar he355_ckks_scalar_residues(Lt + 1, (c_k * T) / s_k);
 *           the constant he355_ckks_scalar_residues(Lt + 1, c_0 * T) when c_0 != 0; ONE he355_combine_scalars at level Lt + 1 over the used
 *           powers, each read at its own level, then he355_rescale to Lt.  A leaf whose powers lie below Lt + 1 is refused.
 *   eval(p, Lt, S), otherwise (a node):  e = the largest giant exponent <= deg p, g = x^e at scale s_g, p = lo + x^e hi, T = S * q[Lt].
 *           hi of degree >= 1:  H = eval(hi, Lt + 1, T / s_g);  prod = he355_multiply_relin(H, drop(g, Lt + 1), rescale = 1)
 *           hi a constant c:    prod = he355_rescale(he355_combine_scalars(Lt + 1, {g}, scalar (c * T) / s_g))       (no product)
 *           lo all zero: prod.  lo a constant c_0: he355_combine_scalars(Lt, {prod}, scalar 1, constant c_0 * S).  else prod + eval(lo, Lt, S).
 *           The nominal scale of the result is exactly S.
 *   depth   leaf: 1 + max over used k >= 1 of ceil(log2 k).  node: max(1 + max(depth(hi), ceil(log2 e)) -- 1 + ceil(log2 e) for a
 *           constant hi --, depth(lo) for a lo of degree >= 1).  The call is eval(p, L - depth, out_scale).
 *           log_baby = 1 gives the least depth, ceil(log2(deg + 1)); a larger baby side costs one more level at some degrees and saves
 *           ciphertext products: he355_ckks_eval_poly_plan states the trade.
 * n is processed in the key-switch chunk.  The power store and the node temporaries are ONE block taken from the context's pool after the
 * relinearization-key check and before the first launch (the allocator's error if it does not fit; nothing is launched then).
 * Refused on the host before any device work: a BFV context, L outside 1..L_top, no non-zero coefficient above c_0, more than 1024
 * coefficients, log_baby outside 1..6, a non-finite coefficient, a scale that is non-finite or <= 0, depth >= L, a scalar
 * he355_ckks_scalar_residues refuses, d_out overlapping d_in, null pointers with work to do.  A missing relinearization key is
 * "relinearization key not present", said before anything is allocated.  n == 0 touches nothing. */
typedef struct he355_poly_plan {
    int32_t depth, L_out;     /* levels the call consumes; the level of d_out = L - depth                                        */
    int32_t min_scalar_bits;  /* the least floor(log2 |a|) over the non-zero integer scalars of leaves: the caller's precision check
                               * (a scalar of b bits carries its coefficient to about 2^-b); -1: every scalar rounded to zero       */
    int32_t degree;           /* after trimming                                                                                   */
    uint64_t products;        /* he355_multiply_relin calls per chunk: power tree + nodes                                          */
    uint64_t combinations;    /* k_scalar_combine launches per chunk                                                              */
    uint64_t rescales;        /* he355_rescale calls per chunk (leaves; the products carry their own)                              */
    uint64_t drops, adds;     /* he355_mod_switch_drop copies and he355_add calls per chunk                                        */
    uint64_t powers;          /* powers computed, x^1 not counted                                                                  */
    uint64_t chunks;          /* ceil(n / min(n, batch chunk)): he355_poly_stats grows by chunks * the counts above                */
    uint64_t pool_bytes;      /* an upper bound of the pool bytes the call takes at the context's batch chunk; 0 for n == 0        */
    double out_scale;         /* the nominal scale of d_out: out_scale as given                                                    */
    uint64_t power_mask[16];  /* bit k: x^k is computed (k >= 2)                                                                    */
    uint64_t reserved[5];
} he355_poly_plan_t;          /* 256 bytes */
int he355_ckks_eval_poly_plan(const he355_ctx *ctx, int L, const double *h_coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                              uint64_t n, he355_poly_plan_t *out);
int he355_ckks_eval_poly(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in /* [n][2][L][N] */, const double *h_coeffs, uint64_t n_coeffs, int log_baby,
                         double in_scale, double out_scale, uint64_t *d_out /* [n][2][L - depth][N] */);
/* What he355_combine_scalars and he355_ckks_eval_poly of this context ran since he355_device_init (or the last call with reset != 0);
 * he355_path_stats counts the products' key switches as for any he355_multiply_relin, he355_hoist_stats nothing. */
typedef struct he355_poly_stats {
    uint64_t combinations; /* k_scalar_combine launches (he355_combine_scalars: one per call with work)   */
    uint64_t products;     /* he355_multiply_relin calls made by he355_ckks_eval_poly, per chunk           */
    uint64_t rescales;     /* he355_rescale calls made by it, per chunk                                    */
    uint64_t drops, adds;  /* he355_mod_switch_drop copies / he355_add calls made by it, per chunk         */
    uint64_t chunks;       /* chunks he355_ckks_eval_poly walked                                           */
    uint64_t calls;        /* he355_ckks_eval_poly / he355_ckks_eval_poly_complex calls with work          */
    uint64_t complex_combinations; /* k_scalar_combine_cplx launches; `combinations` does not count them   */
} he355_poly_stats_t;
int he355_poly_stats(he355_ctx *ctx, he355_poly_stats_t *out, int reset);
/* ---- complex CKKS slots: codec, complex scalars and complex polynomial coefficients ----
 * The encoders place slot j at zeta^(3^j) (SEAL's slot map).  Because 3 = 3 (mod 4), X^(N/2) evaluates to i * (-1)^j in slot j: it is NOT
 * "multiply by i".  What exists is J(X) = X^(N/4) + X^(3N/4):
 *   J decodes to sqrt(2) * i in EVERY slot, exactly;
 *   NTT_{q_i}(J)[e] = u_i when bit (log2 N - 2) of the NTT index e is 0, and q_i - u_i when it is 1;  u_i = NTT_{q_i}(J)[0],  u_i^2 = -2 (mod q_i).
 * So a complex constant at weight W is the integer polynomial A + B * J, A = rint(Re * W), B = rint(Im * W / sqrt(2)): in NTT form ONE of two
 * residues per prime, A +- B * u_i, chosen by s(e) = bit (log2 N - 2) of e.  Like every scalar of he355_ckks_eval_poly it carries its scale.
 *
 * he355_ckks_encode_complex: he355_ckks_encode with d_values [n][count][2] doubles (re, then im): z[slot_index[i]] = v and
 *   z[slot_index[N/2 + i]] = conj(v); everything else is the shared code of client/ckks_codec.h in the same order of IEEE operations, with
 *   the same overflow refusal ("encoded values are too large": a non-finite value ends there).  Values with im = +0.0 give the residues of
 *   he355_ckks_encode bit for bit (the signed zeros of the conjugate reach only results that are zero).
 * he355_ckks_decode_complex / _slots: d_out [n][N/2][2] / [n][sum of counts][2]; the re parts are the bits of he355_ckks_decode /
 *   he355_ckks_decode_slots, the im parts the .im the transform already holds.  The same two kernels, then one gather of the wanted pairs.
 * Both agree with client::Client::ckks_encode_complex / ckks_decode_complex (the host client, csrc/client/he_client.h) bit for bit.
 * Refused on the host before any device work (HE355_E_INVALID_ARGS, the message names the call): a BFV context, count > N/2, L outside
 * 1..L_top or above 16, a scale that is not finite and positive, 0 or more than 4 ranges or one outside the N/2 slots, null pointers with
 * work to do, slabs past 2^60 words or wrapping the address space.  n == 0 touches nothing. */
int he355_ckks_encode_complex(he355_ctx *ctx, uint64_t n, const double *d_values /* [n][count][2] */, uint64_t count, double scale,
                              uint64_t *d_plain /* [n][L_top][N], NTT form */);
int he355_ckks_decode_complex(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain, double scale, double *d_out /* [n][N/2][2] */);
int he355_ckks_decode_complex_slots(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain, double scale, const uint64_t *ranges, uint64_t n_ranges,
                                    double *d_out /* [n][sum of counts][2] */);
/* Host only: out[i] = u_i.  Refused: L outside 1..L_top, null out. */
int he355_ckks_complex_unit(const he355_ctx *ctx, int L, uint64_t *out /* [L] */);
/* Host only: A = the integer of he355_ckks_scalar_residues(v_re), B = that of v_im / sqrt(2.0) (an IEEE division: Python's
 * v_im / math.sqrt(2.0)); out[0][i] = (A + B * u_i) mod q_i, out[1][i] = (A - B * u_i) mod q_i, canonical.  Refuses what
 * he355_ckks_scalar_residues refuses, for either part. */
int he355_ckks_complex_scalar_residues(const he355_ctx *ctx, int L, double v_re, double v_im, uint64_t *out /* [2][L] */);
/* he355_combine_scalars with the scalar and the constant picked per NTT index:
 *   out[c][k][i][e] = (sum_t h_scalars[t][s(e)][i] * term_t[c][k][i][e] + (k == 0 ? h_const[s(e)][i] : 0)) mod q_i,  s(e) = bit (log2 N - 2) of e
 * Any pair of canonical residues is allowed, not only A +- B * u.  Terms, levels, strides, the overlap rules, the 2^20-term cap, the table
 * ring and every refusal are he355_combine_scalars', under this call's name; with both halves equal it gives that call's bits.  One
 * streaming launch of k_scalar_combine_cplx (he355_poly_stats: complex_combinations). */
int he355_combine_scalars_complex(he355_ctx *ctx, int L, int size, uint64_t n, const he355_term *h_terms, uint64_t n_terms,
                                  const uint64_t *h_scalars /* [n_terms][2][L] canonical residues */, const uint64_t *h_const /* [2][L] or NULL */,
                                  uint64_t *d_out /* [n][size][L][N] */);
/* he355_ckks_eval_poly with complex coefficients c_k = h_re[k] + i * h_im[k] (both lists n_coeffs long).  The tree, the depth, the power
 * set, the levels and the products are he355_ckks_eval_poly's; a coefficient is zero when both of its parts are.  Every scalar
 * (c_k * T) / s_k becomes the pair ((re_k * T) / s_k, (im_k * T) / s_k) given to he355_ckks_complex_scalar_residues, every constant c * T
 * or c * S a pair in the same way; every leaf and every constant combination is ONE he355_combine_scalars_complex.  The plan's
 * `combinations` counts those launches (he355_poly_stats: complex_combinations grows by them, combinations by none); min_scalar_bits is
 * the least over the non-zero integers A and B.  With h_im all zero the output equals he355_ckks_eval_poly's bit for bit.  The input slots
 * may themselves be complex.  Refusals: he355_ckks_eval_poly's under this call's name, and a null h_im. */
int he355_ckks_eval_poly_complex_plan(const he355_ctx *ctx, int L, const double *h_re, const double *h_im, uint64_t n_coeffs, int log_baby, double in_scale,
                                      double out_scale, uint64_t n, he355_poly_plan_t *out);
int he355_ckks_eval_poly_complex(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in /* [n][2][L][N] */, const double *h_re, const double *h_im,
                                 uint64_t n_coeffs, int log_baby, double in_scale, double out_scale, uint64_t *d_out /* [n][2][L - depth][N] */);
/* ---- the modulus raise (CKKS): from q_0 alone back up the chain, on a fused lift-and-transform kernel ----
 * Every other level operation goes down (he355_rescale, he355_mod_switch_drop); this one takes a ciphertext whose chain is used up back to
 * L_to primes, the first step of a bootstrapping circuit.  The definition (tests/ckks_mod_raise_ref.py restates it on the oracle), for every
 * polynomial p of the n * size:
 *   x   = iNTT_{q_0}(in[p][0])                                    (coefficients, canonical under q_0)
 *   c_e = x_e if x_e <= (q_0 - 1) / 2, else x_e - q_0             (the centred integer: he355_plain_extend_special's range)
 *   out[p][j] = NTT_{q_j}(c mod q_j), canonical, j < L_to
 * so the raised ciphertext decrypts over q_0 .. q_{L_to - 1} to m + q_0 * I with a small integer polynomial I (|I| <= (h + 2) / 2 for a
 * ternary secret of Hamming weight h); removing q_0 * I is the circuit's business (linear transforms, he355_ckks_eval_poly).
 * Only row 0 of the input is read, with the input's own [L_in][N] stride: rows >= 1 are ignored (he355_mod_switch_drop's rule, no copy).
 * out[p][0] is in[p][0] bit for bit, made by a copy.  L_to = 1 is that copy alone; L_to > L_in is the use; L_to <= L_in means the same.
 * The call equals, bit for bit, the composition of public calls: copy row 0, he355_ntt_inverse (prime 0), he355_ckks_lift_centred,
 * he355_ntt_forward (primes 0 .. L_to - 1) -- without the coefficient slab and the lifted slab in memory: N >= 2048 runs the inverse row
 * pass of row 0 into a compact tail, ONE kernel that finishes the inverse transform of a column, lifts it and runs the forward column pass
 * per target (k_raise_cols), and the forward row pass in place; N = 1024, which has no column pass, runs inverse transform ->
 * k_raise_lift -> forward transform.  n is processed in the key-switch chunk (he355_set_chunk).  A chunk of nc ciphertexts with
 * nc * size * 4 below the device's compute-unit count deals the targets of a column to
 * tsplit = min(L_to - 1, ceil(CUs / (nc * size * 4))) blocks (he355_set_latency_max(0) switches this off with the other latency shapes).
 * he355_ckks_lift_centred is the middle step on its own: d_coeff [n_polys][N], coefficients canonical under q_0 -> d_out [n_polys][L_to][N],
 * row j = c mod q_j, canonical, coefficient form (row 0 = the input).  One streaming launch.
 * Refused on the host before any device work (HE355_E_INVALID_ARGS, the message names the call): a BFV context, L_in or L_to outside
 * 1..L_top, size outside 1..3, null pointers with work to do, slabs past 2^60 words or wrapping the address space, d_out overlapping any
 * word of d_in (its ignored rows count) or of d_coeff, a slab that is not 16-byte aligned (the kernels move two words at a time; an offset
 * of whole polynomials into an aligned slab stays aligned).  n == 0 touches nothing and needs no device. */
int he355_ckks_mod_raise(he355_ctx *ctx, int L_in, int L_to, int size, uint64_t n, const uint64_t *d_in /* [n][size][L_in][N], NTT form */,
                         uint64_t *d_out /* [n][size][L_to][N], NTT form */);
int he355_ckks_lift_centred(he355_ctx *ctx, int L_to, uint64_t n_polys, const uint64_t *d_coeff /* [n_polys][N], coefficients, canonical under q_0 */,
                            uint64_t *d_out /* [n_polys][L_to][N], coefficients */);
/* What the two calls of this context ran since he355_device_init (or the last call with reset != 0); he355_path_stats, he355_hoist_stats
 * and he355_poly_stats count nothing of them. */
typedef struct he355_raise_stats {
    uint64_t calls;              /* he355_ckks_mod_raise calls with work                                             */
    uint64_t chunks;             /* chunks they walked                                                               */
    uint64_t fused_launches;     /* k_raise_cols launches (N >= 2048, L_to >= 2: one per chunk)                      */
    uint64_t streaming_launches; /* k_raise_lift launches (N = 1024 with L_to >= 2: one per chunk; he355_ckks_lift_centred: one) */
    uint64_t split_launches;     /* the fused launches that dealt a column's targets to tsplit > 1 blocks            */
    uint64_t reserved[3];
} he355_raise_stats_t;           /* 64 bytes */
int he355_raise_stats(he355_ctx *ctx, he355_raise_stats_t *out, int reset);
/* ---- EvalMod (CKKS): Chebyshev-basis evaluation on a fused combine-and-rescale step ----
 * he355_combine_scalars_rescale equals, bit for bit, he355_combine_scalars into a temporary [n][size][L][N] followed by he355_rescale:
 *   d_out [n][size][L - 1][N] = rescale(sum_t a_t * ct_t + a_const)
 * without the temporary.  Per chunk (the key-switch chunk, he355_set_chunk): row L - 1 of the combination alone into a compact pool block
 * (k_scalar_combine_row), its inverse row pass and the floor step's column half exactly as he355_rescale runs them (with its latency split;
 * he355_set_latency_max(0) switches that off), then ONE row kernel (k_floor_rows_combine) that forms the sums of rows 0 .. L - 2 from the
 * term rows themselves -- each term read with its own [L_t][N] stride, integer sums under every prime -- and finishes the floor step on
 * them.  There is no ring-in-LDS form and no dual-engine launch; the bits are he355_rescale's in whichever form that call takes.
 * Refused on the host before any device work (the message names this call): everything he355_combine_scalars refuses, L < 2, a BFV context,
 * d_out [n][size][L - 1][N] overlapping any word of any term.  n == 0, or n_terms == 0 without a constant, touches nothing. */
int he355_combine_scalars_rescale(he355_ctx *ctx, int L, int size, uint64_t n, const he355_term *h_terms, uint64_t n_terms,
                                  const uint64_t *h_scalars /* [n_terms][L] canonical residues */, const uint64_t *h_const /* [L] or NULL */,
                                  uint64_t *d_out /* [n][size][L - 1][N] */);
/* he355_ckks_eval_chebyshev: out = p(u), p(u) = sum_k c_k T_k(u) (Chebyshev polynomials of the first kind, real coefficients, trailing zeros
 * trimmed), u the input at in_scale, assumed in [-1, 1].  An affine map from [a, b] is the caller's: subtract the constant (a + b) / 2 with
 * he355_combine_scalars and pass in_scale * (b - a) / 2 as in_scale.  Arguments, levels, chunking, memory and refusals are
 * he355_ckks_eval_poly's; one more refusal: a coefficient that becomes non-finite in a split.  The monomial tree cannot serve here: the
 * monomial coefficients of a degree 15..63 cosine on [-K, K] are too ill-conditioned at this library's scales, and a Chebyshev step must
 * subtract BEFORE the rescale -- which is he355_combine_scalars_rescale.
 * The definition (tests/ckks_eval_mod_ref.py restates it on the oracle).  All scale arithmetic is IEEE double in the order written;
 * scalar_residues is he355_ckks_scalar_residues, drop is he355_mod_switch_drop, q[l] is prime index l.
 *   powers  m = 2^log_baby; babies T_1 .. T_(m-1), giants T_(m 2^j) while the index is <= the degree.  The needed set is
 *           he355_ckks_eval_poly's, closed under the halves a = ceil(k/2), b = floor(k/2).  T_1 = the input, level L, scale s_1 = in_scale.
 *           For k >= 2 in increasing order:  l = min(level_a, level_b);  W = s_a * s_b;
 *             P = he355_multiply_relin(drop(T_a, l), drop(T_b, l), rescale = 0);
 *             k even:  T_k = he355_combine_scalars_rescale(l, {P}, scalar 2, constant scalar_residues(l, -W));
 *             k odd:   T_k = he355_combine_scalars_rescale(l, {P, T_1 read at level L}, scalars {2, scalar_residues(l, -(W / s_1))});
 *           T_k lies at level l - 1 with scale s_k = W / q[l - 1].  (T_(a+b) = 2 T_a T_b - T_(a-b); with halves a - b is 0 or 1.)
 *   eval(p, Lt, S), deg p < m (a leaf):  he355_ckks_eval_poly's leaf verbatim -- T = S * q[Lt], scalars (c_k * T) / s_k, constant c_0 * T --
 *           as ONE he355_combine_scalars_rescale at level Lt + 1.
 *   eval(p, Lt, S), otherwise (a node):  e = the largest giant <= deg p.  The split is in the Chebyshev basis: hi[0] = c_e;
 *           lo = c_0 .. c_(e-1); for k = e + 1 .. deg in increasing order hi[k - e] = 2.0 * c_k and lo[2e - k] = lo[2e - k] - c_k; lo is
 *           trimmed (a coefficient that cancels to 0.0 is zero).  Then he355_ckks_eval_poly's node rule unchanged, with g = T_e:
 *           H = eval(hi, Lt + 1, T / s_g) and the product with rescale = 1; a constant hi is a one-term leaf of T_e; a constant lo is a
 *           he355_combine_scalars with scalar 1 and the constant; otherwise he355_add.
 *   depth   he355_ckks_eval_poly's formulas on the split above; the call is eval(p, L - depth, out_scale).
 * The plan reuses he355_poly_plan_t: `rescales` counts the fused steps, `combinations` the he355_combine_scalars launches, pool_bytes
 * includes the fused steps' row block. */
int he355_ckks_eval_chebyshev_plan(const he355_ctx *ctx, int L, const double *h_coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                                   uint64_t n, he355_poly_plan_t *out);
int he355_ckks_eval_chebyshev(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in /* [n][2][L][N] */, const double *h_coeffs, uint64_t n_coeffs, int log_baby,
                              double in_scale, double out_scale, uint64_t *d_out /* [n][2][L - depth][N] */);
/* he355_ckks_eval_mod: y_0 = p(u) by he355_ckks_eval_chebyshev, then r = double_angles (0..8) steps y <- 2 y^2 - 1.  The depth is
 * depth(p) + r and must be below L; d_out lies at level L - depth(p) - r.
 *   scales  l_0 = L - depth(p), l_j = l_0 - j.  S_r = out_scale; backwards S_(j-1) = sqrt(S_j * q[l_j]) (the IEEE square root); the
 *           Chebyshev part runs at the target S_0.  Forwards s_0 = S_0, s_j = (s_(j-1) * s_(j-1)) / q[l_j].
 *   step j  z = he355_multiply_relin(y, y, rescale = 1);  y_j = he355_combine_scalars(l_j, {z}, scalar 2, constant scalar_residues(l_j, -s_j)).
 * The plan's out_scale is s_r, the scale d_out carries: out_scale up to rounding.  Its products and combinations include the steps', and
 * reserved[0] holds double_angles.  With r = 0 the call gives he355_ckks_eval_chebyshev's bits.
 * Use.  After he355_ckks_mod_raise a ciphertext holds t = m + q_0 * I with |I| < K.  Pass h_coeffs = the Chebyshev interpolant of
 * cos((2 pi / 2^r) (K u - 1/4)) on [-1, 1] and in_scale = q_0 * K (then u = t / (q_0 K)); after the r double angles the result is
 * cos(2 pi t / q_0 - pi / 2) = sin(2 pi t / q_0) ~ 2 pi m / q_0 at out_scale, so a message at scale Delta is read at scale
 * out_scale * 2 pi Delta / q_0.  The C ABI takes coefficients only, so that no libm call is part of a bit-exact definition.
 * The powers' scales follow s_k = s_a * s_b / q[l - 1]: they stay put when in_scale is about the size of the primes the powers rescale by
 * and grow with k when it is far above them, until a scalar passes 2^126 and the call is refused -- so EvalMod's levels take primes near
 * q_0 * K, as bootstrapping chains do (in_scale = 12 * q_0 over 45-bit primes is refused from degree 16 on). */
int he355_ckks_eval_mod_plan(const he355_ctx *ctx, int L, const double *h_coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                             int double_angles, uint64_t n, he355_poly_plan_t *out);
int he355_ckks_eval_mod(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_in /* [n][2][L][N] */, const double *h_coeffs, uint64_t n_coeffs, int log_baby,
                        double in_scale, double out_scale, int double_angles, uint64_t *d_out /* [n][2][L - depth - r][N] */);
/* What the three calls above ran on this context since he355_device_init (or the last call with reset != 0).  he355_poly_stats does not
 * move for them; he355_path_stats counts the products' key switches as for any he355_multiply_relin. */
typedef struct he355_cheb_stats {
    uint64_t calls;         /* he355_ckks_eval_chebyshev / he355_ckks_eval_mod calls with work                              */
    uint64_t chunks;        /* chunks they walked                                                                           */
    uint64_t products;      /* he355_multiply_relin calls they made, per chunk (the double angles' squares included)         */
    uint64_t fused_steps;   /* combine-and-rescale sequences, per chunk; he355_combine_scalars_rescale: one per call         */
    uint64_t combinations;  /* k_scalar_combine launches they made, per chunk (constant lows, double angles)                 */
    uint64_t drops, adds;   /* he355_mod_switch_drop copies / he355_add calls they made, per chunk                           */
    uint64_t double_angles; /* steps y <- 2 y^2 - 1, per chunk                                                               */
} he355_cheb_stats_t;       /* 64 bytes */
int he355_cheb_stats(he355_ctx *ctx, he355_cheb_stats_t *out, int reset);
/* accumulateCKKS / accumulateBFV: in place log-tree sum of the first `count` slots; d_tmp: scratch slab of the same size.
 * count == 0 is the reference's else-branch (src/engine/seal_context.cpp:312-316, 341-344): every ciphertext is replaced by a
 * FRESH encryption of zero (Encryptor::encrypt_zero; needs the public key; L must be the top level, as SEAL returns a
 * top-level ciphertext there).  The randomness comes from the context's own stream: seeded from the OS, or pinned with
 * he355_set_zero_stream (ciphertext r then equals he355_encrypt_zero(seed, first_index + r)). */
int he355_accumulate(he355_ctx *ctx, int L, uint64_t n, uint64_t *d_inout, uint64_t count, uint64_t *d_tmp);
/* Encryptor::encrypt_zero at the first data level: d_out [n][2][Ltop][N]; streams as he355_encrypt */
int he355_encrypt_zero(he355_ctx *ctx, uint64_t n, uint64_t seed, uint64_t first_index, uint64_t *d_out);
int he355_set_zero_stream(he355_ctx *ctx, uint64_t seed, uint64_t first_index);
/* Introspection: the API-Bridge ABI (enumerators, sizes, offsets, header used) this library was compiled with, as JSON; returns the
 * size needed including the terminator (csrc/bridge/abi_check.cpp).  A harness binding can check its own numbers against it. */
uint64_t he355_bridge_abi(char *p_buffer, uint64_t size);
/* Introspection: bytes the most recent multi-device load() of the bridge moved to device `device` (> 0) for operand 0 / 1
 * (csrc/bridge/multi_device.cpp): operand 0 travels in per-device blocks, operand 1 whole. */
uint64_t he355_bridge_group_load_bytes(int device, int operand);
/* ---- client side on the device: encryptor()->encrypt (ckks eltwise .cpp:242, bfv eltwise .cpp:233) and
 * SEALContextWrapper::decrypt (src/engine/seal_context.cpp:265-287), batched.  Keys: host arrays in SEAL layout, NTT form:
 * public key [2][K][N], secret key [K][N].  Randomness of he355_encrypt is counter-based: ciphertext r draws u, e0, e1 from
 * (seed, index first_index + r) — csrc/client/sampler.h — so the host client with the same seed/index gives the same bits. */
int he355_set_public_key(he355_ctx *ctx, const uint64_t *h_pk);
int he355_set_secret_key(he355_ctx *ctx, const uint64_t *h_sk);
/* d_plain: CKKS [n][L_top][N] NTT-form plaintexts, BFV [n][N] coefficients mod t; d_out: [n][2][L_top][N] */
int he355_encrypt(he355_ctx *ctx, uint64_t n, const uint64_t *d_plain, uint64_t seed, uint64_t first_index, uint64_t *d_out);
/* d_ct: [n][size][L][N], size 2 or 3; d_out: CKKS [n][L][N] NTT-form plaintext, BFV [n][N] coefficients mod t */
int he355_decrypt(he355_ctx *ctx, int L, int size, uint64_t n, const uint64_t *d_ct, uint64_t *d_out);
/* Encoders on the device: CKKSEncoder()->encode / decode and BatchEncoder (src/engine/seal_context.cpp:145-185 and the
 * benchmarks' encode()/decode(), e.g. src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:163-226).  All pointers are device
 * pointers.  CKKS: values [n][count] doubles (count <= N/2, missing slots are 0) -> [n][L_top][N] NTT-form plaintexts at `scale`;
 * decode: [n][L][N] -> [n][N/2] real parts.  BFV: values [n][count] int64 <-> [n][N] coefficients mod t (centred on decode). */
int he355_ckks_encode(he355_ctx *ctx, uint64_t n, const double *d_values, uint64_t count, double scale, uint64_t *d_plain);
int he355_ckks_decode(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain, double scale, double *d_out);
int he355_bfv_encode(he355_ctx *ctx, uint64_t n, const int64_t *d_values, uint64_t count, uint64_t *d_plain);
int he355_bfv_decode(he355_ctx *ctx, uint64_t n, const uint64_t *d_plain, int64_t *d_out);
/* The same decoders writing only the slots a caller reads: `ranges` = n_ranges (1..4) HOST pairs {first_slot, count}; d_out is
 * [n][sum of counts], the ranges one after the other.  A workload's decode() copies the first n (vectors) or dim3 (matrix rows) slots of
 * each result (src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:214-226; both batching rows for the BFV row-major product,
 * bfv/seal_bfv_matmult_row_benchmark.cpp:339-369), so the device writes and the host downloads n x count values instead of n x N/2 (N). */
int he355_ckks_decode_slots(he355_ctx *ctx, int L, uint64_t n, const uint64_t *d_plain, double scale, const uint64_t *ranges, uint64_t n_ranges, double *d_out);
int he355_bfv_decode_slots(he355_ctx *ctx, uint64_t n, const uint64_t *d_plain, const uint64_t *ranges, uint64_t n_ranges, int64_t *d_out);
/* Page-locked host memory (hipHostMalloc) for he355_upload / he355_download of small, frequent transfers (the bridge's decode results and
 * encode inputs live in one such buffer per benchmark object). */
int he355_host_alloc(he355_ctx *ctx, uint64_t bytes, void **h_ptr);
int he355_host_free(he355_ctx *ctx, void *h_ptr);
/* transforms of n_polys residue polynomials, polynomial p under prime prime_of[p % period] (test / client use) */
int he355_ntt_forward(he355_ctx *ctx, uint64_t *d_polys, uint64_t n_polys, const uint8_t *prime_of, uint32_t period);
int he355_ntt_inverse(he355_ctx *ctx, uint64_t *d_polys, uint64_t n_polys, const uint8_t *prime_of, uint32_t period);

/* ---- timing on the stream the kernels run on (HIP events) ---- */
int he355_timer_begin(he355_ctx *ctx);
int he355_timer_end(he355_ctx *ctx, float *elapsed_ms);
/* HIP events around every launch of the dominant kernel (k_k3, fp64-engine primes: the key-product kernel of the key switch)
 * between he355_timer_begin and he355_timer_end: summed duration, number of launches and ops they covered */
int he355_probe_dominant_kernel(he355_ctx *ctx, float *total_ms, uint64_t *launches, uint64_t *ops);
/* Shader clock held while a region runs: he355_clock_probe_begin launches one 64-lane wave on a stream of its own that samples the
 * shader-cycle counter against the constant 100 MHz counter for `duration_us` of real time (a bound it always reaches) while whatever
 * is queued next runs beside it; he355_clock_probe_end waits for it: *mhz = cycles / real time, *seconds = the time it covered.
 * (bench.py: the VALU-issue roofline needs the clock the chip held under THIS load, not a nominal one.) */
int he355_clock_probe_begin(he355_ctx *ctx, uint64_t duration_us);
int he355_clock_probe_end(he355_ctx *ctx, double *mhz, double *seconds);
/* ---- tuning ---- */
int he355_set_dual_stream(he355_ctx *ctx, int on); /* chunks alternate between two HIP streams (default 1; HE355_DUAL_STREAM=0); 0: per-kernel timings without overlap */
/* Key switches over at most n ciphertexts take the latency shape (serial loops of the throughput kernels dealt to more blocks; HEBench's
 * Latency category is batch 1: src/benchmarks/ckks/seal_ckks_element_wise_benchmark.cpp:138-141).  Default: 2^17 / N ciphertexts, at most 12 -- where the throughput kernels start filling the chip (4 at N = 2^15, 8 at 2^14);
 * a call (or HE355_LATENCY_MAX) replaces the rule by n; 0: never; UINT64_MAX: the rule again.
 * Results are bit-identical either way. */
int he355_set_latency_max(he355_ctx *ctx, uint64_t n);
/* he355_rotate_sum walks its NAF-prefix trie level by level, all nodes of a level in one grouped key-switch sequence (default 1;
 * HE355_LEVEL_WALK=0), or node by node (0: one sequence per node; what CKKS batches within the latency shape always take).  Results are
 * bit-identical either way. */
int he355_set_level_walk(he355_ctx *ctx, int on);
/* Rings that fit one CU's LDS (N <= 8192, at most 6 data primes: L <= 6): key switches over at most n ciphertexts per kernel sequence run as TWO
 * launches of one-polynomial workgroups whose transforms never leave LDS (csrc/he355_kernels_lds.hip; the reference's descriptors default
 * to N = 8192: src/benchmarks/ckks/seal_ckks_dot_product_benchmark.cpp:53-60).  Default: the library's rule (one and a half rounds of the chip for the first kernel's grid: 64 ciphertexts at {60, 40, 60}); a call (or
 * HE355_LDS_MAX) replaces it by n; 0: never; UINT64_MAX: the rule again.  Results are bit-identical either way. */
int he355_set_lds_max(he355_ctx *ctx, uint64_t n);
/* ops processed per kernel sequence: default 1024 (HE355_CHUNK), i.e. BASELINE configs[2]'s batch in one piece (scratch ~ 117 MiB/op at
 * N=2^15, L=16).  The size actually used is halved until the scratch arena(s) fit in the device memory that is free at the call. */
int he355_set_chunk(he355_ctx *ctx, uint64_t ops_per_chunk);
int he355_mem_info(he355_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes); /* hipMemGetInfo of the context's device */

#ifdef __cplusplus
}
#endif
#endif
