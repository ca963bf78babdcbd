// he355_launchers.inc -- prototypes of the host-callable launchers, included by he355_kernels.h once per build of the device code
// (namespace ks_shoup: the u64 engine multiplies by constants through Shoup quotients; namespace ks_fold: through the fold reduction
// for primes 2^60 - c, modarith.h).  Every he355_kernels*.hip is compiled twice, each time into one of the two.
// ---- generic transforms over a PolyView (in place) ---------------------------------------------------
void launch_ntt_forward(const KernelEnv &env, const PolyView &v, u32 n_items);  // canonical -> canonical NTT form
void launch_ntt_inverse(const KernelEnv &env, const PolyView &v, u32 n_items);  // canonical NTT form -> coefficients
// ---- element-wise ------------------------------------------------------------------------------------
// out[r][p][n] = a[ia(r)][p][n] (+|-) b[ib(r)][p][n] mod q_{p % L}; polys = size * L
void launch_addsub(const KernelEnv &env, int L, int size, u64 n_results, const u64 *a, const u64 *b, Indexer ix, u64 *out, bool sub);
// dyadic tensor (CKKS multiply): a,b size-2 level-L NTT form -> out size 3
void launch_mul3(const KernelEnv &env, int L, u64 n_results, const u64 *a, const u64 *b, Indexer ix, u64 *out);
void launch_plain_op(const KernelEnv &env, int L, int size, u64 n_results, const u64 *ct, const u64 *pt, Indexer ix, u64 *out, int mode); // 0 mul, 1 add
void launch_drop_residues(const KernelEnv &env, int L, int L_to, u64 n_polys, const u64 *in, u64 *out);
// out[c] (+)= sum_r in[r * n_out + c], c < n_out
void launch_sum_cts(const KernelEnv &env, int L, int size, u64 n_terms, const u64 *in, u64 *out, u64 n_out = 1, bool accumulate = false);
void launch_mul3_acc(const KernelEnv &env, int L, u64 rows, u64 cols, int inner, const u64 *a, u64 a_stride_i, u64 a_stride_k, const u64 *b,
                     u64 b_stride_k, u64 b_stride_j, u64 *out);
// out[c] += sum_g mult[g] * in[g * n_cts + c] over size-2 ciphertexts at level L (d_mult: device array [n_groups])
void launch_sum_groups(const KernelEnv &env, int L, u64 n_cts, u32 n_groups, const u64 *in, const u32 *d_mult, u64 *out);
// whole ciphertexts by index list (host array): gather dst[g] = src[idx[g]], scatter dst[idx[g]] = src[g], g < n
void launch_move_cts(const KernelEnv &env, u64 *dst, const u64 *src, const uint32_t *idx, u64 n, u64 elems_per_ct, bool scatter);
// K1: produce c01 / c2n / c2r for a chunk of n_ops ops from the operands `src` names (K1Operands, he355_kernels.h)
void launch_k1(const KernelEnv &env, int L, u64 n_ops, const K1Operands &src, const KsBuffers &buf);
// K2: finish iNTT of each digit, lift to every key prime, forward column pass -> d
// src_is_coeff (BFV): `src` already holds coefficient-form digits [op][L][N] (op stride src_op_stride) and every
// (prime, digit) pair is lifted, including the digit's own prime
// tsplit > 1 (latency shape, k_k2n): the targets of a (digit, column block) are dealt to tsplit blocks
void launch_k2(const KernelEnv &env, int L, u64 n_ops, const KsBuffers &buf, const u64 *src = nullptr, u64 src_op_stride = 0, int tsplit = 1);
// n_split > 1 (latency shape, unfused only): the digits of every tile are cut into n_split groups, one single-wave block per (tile, op,
// group), canonical partial sums -> split_part [n_split][n_ops * 2][L + 1][N]; launch_k3_combine then leaves t / tpr as the unsplit launch
void launch_k3(const KernelEnv &env, int L, u64 n_ops, const KsBuffers &buf, const u64 *key, K3Part part = K3_ALL, const K3Fuse *fuse = nullptr,
               int n_split = 1, u64 *split_part = nullptr, int n_split_u64 = 0, // n_split_u64: groups of the u64-engine tiles (0: as n_split)
               const KsGroups *groups = nullptr, u64 g_op_offset = 0);         // groups: per-group keys (`key` unused), op 0 of the launch is op g_op_offset of the grouped batch
void launch_k3_combine(const KernelEnv &env, int L, u64 n_ops, const KsBuffers &buf, int n_split, const u64 *split_part, int n_split_u64 = 0);
// floor step, column half: src [n_ops*n_src][N] raw of prime s -> r = (x + floor(s/2)) mod s ->
// (r mod q_i - floor(s/2) mod q_i) for i in [tgt_first, tgt_first + n_tgt) -> forward column pass -> dst [n_ops*n_src][dst_ntgt][N]
// src2 (optional): the SOURCE of an earlier floor step ([n_polys][N] after its inverse row pass, prime src2_prime): its correction is
// folded in before the column pass, delta2 + src2^-1 * delta1 (mod-down + rescale share one column pass and one row transform)
// sub2 (with src2): src still lacks the earlier correction under its own prime (K3Fuse::raw_tail rows); x - src2^-1 * delta1 mod q_src is
// formed first, once per column
void launch_floor_cols(const KernelEnv &env, int src_prime, int n_tgt, u64 n_polys, const u64 *src, u64 *dst, int tgt_first = 0, int dst_ntgt = 0,
                       const u64 *src2 = nullptr, int src2_prime = 0, int tsplit = 1, bool sub2 = false);
void launch_floor_rows(const KernelEnv &env, u64 n_ops, const FloorRowsArgs &args);
// ---- BFV -------------------------------------------------------------------------------------------------
// (BehzDev, kBehzMaxL / kBehzMaxB and the per-coefficient BEHZ arithmetic: behz_core.h -- host-compilable, the lane simulator runs it on the CPU)
// BEHZ steps (1)-(2): lift the four input polynomials of each pair to Bsk (fastbconv_m_tilde + sm_mrq) and copy them
// for the base-q transform.  xq [n*4][L][N], xbsk [n*4][S][N], coefficient form.
// results op_offset .. op_offset + n_ops - 1 of the batch (the indexer sees the global result index)
// n_cts ciphertext items selected by `src` (device_types.h, BehzSrc: the two operands of every result, or each distinct operand once)
// (the launch_behz_* functions return what they chose -- the <16, 24> instantiation, an EXACT instantiation, one launch for both engines --
// for he355_bfv_multiply_stats; the host counts, no launch reads a counter)
bool launch_behz_extend(const KernelEnv &env, const BehzDev &bz, const BehzSrc &src, u64 n_cts, u64 *xq, u64 *xbsk); // true: <kBehzMaxL, kBehzMaxB>
// N <= 16384, L <= 4, nB <= 6 and (L + nB + 1) N / 2 bytes of LDS within what the device grants one block (behz_cols_lds_limit: the
// LOGN1 = 4 pair is opted in above 64 KiB): the extension with the forward column passes of xq / xbsk in its epilogue,
// and the inverse column passes of dq / ds in the prologue of steps (6)-(8) -- the coefficient-form copies never reach HBM
size_t behz_cols_lds_limit(const KernelEnv &env);
bool behz_cols_fusable(const KernelEnv &env, const BehzDev &bz);
bool launch_behz_extend_cols(const KernelEnv &env, const BehzDev &bz, const BehzSrc &src, u64 n_cts, u64 *xq, u64 *xbsk);
// operands transformed once each (src.lists): dyadic tensor + inverse row pass of results op_offset .. op_offset + n_ops - 1
bool launch_behz_tensor_inv(const KernelEnv &env, const BehzDev &bz, const BehzSrc &src, u64 n_ops, u64 op_offset, const u64 *eq, const u64 *ebsk, u64 *dq,
                            u64 *ds);
void launch_rows_fwd(const KernelEnv &env, const PolyView &v, u32 n_items); // row half of the forward transform, in place
void launch_rows_inv(const KernelEnv &env, const PolyView &v, u32 n_items); // row half of the inverse transform, in place (N = 1024: all of it)
bool launch_behz_cols_floor_sk(const KernelEnv &env, const BehzDev &bz, u64 n_ops, const u64 *dq, const u64 *ds, u64 *out);
// BEHZ steps (3)-(5) on rows, fused: x [n*4][Lx][N] after launch_cols_fwd -> forward row pass of a0, a1, b0, b1, dyadic tensor, inverse row
// pass -> d [n*3][Lx][N] ready for launch_cols_inv (one block = the four rows of one (op, residue, row); no HBM round trip between them)
bool launch_behz_rows_tensor(const KernelEnv &env, const BehzDev &bz, u64 n_ops, const u64 *xq, const u64 *xbsk, u64 *dq, u64 *ds);
void launch_cols_fwd(const KernelEnv &env, const PolyView &v, u32 n_items); // column half of the forward transform, in place
void launch_cols_inv(const KernelEnv &env, const PolyView &v, u32 n_items); // column half of the inverse transform, in place
// BEHZ steps (6)-(8): times t, fast floor, Shenoy-Kumaresan -> out [n][3][L][N]
bool launch_behz_floor_sk(const KernelEnv &env, const BehzDev &bz, u64 n_ops, const u64 *dq, const u64 *ds, u64 *out);
// coefficient-form Galois: c01[op][0] = sigma(in0), c01[op][1] = 0, tgt[op] = sigma(in1); gather table has the sign in bit 31
void launch_bfv_galois(const KernelEnv &env, int L, u64 n_ops, const u64 *in, const uint32_t *gather, u64 *c01, u64 c01_item_stride, u64 *tgt,
                       const u64 *addend = nullptr); // addend [n][2][L][N]: out = addend + rotate(in)
// BFV key-switch tails: finish the inverse transform of the special-prime sums and round (-> rp), then finish every data
// prime's inverse transform, apply the floor step in coefficient form and add into c01
void launch_bfv_tail_sp(const KernelEnv &env, u64 n_polys, const u64 *tpr, u64 *rp);
// c01 = add01 + key-switched part (add01 == nullptr: c01 += ...; relinearize hands the size-3 input's (c0, c1) here, nothing is copied)
void launch_bfv_tail_fin(const KernelEnv &env, int L, u64 n_ops, const u64 *t, const u64 *rp, u64 *c01, u64 c01_item_stride, const u64 *add01 = nullptr,
                         u64 add01_item_stride = 0);
// ---- hoisted rotations (he355_kernels_hoist.hip) -----------------------------------------------------------
// dst = the n_polys residue polynomials of src (an installed key and its quotient block), element e of each taken from perm[e]
void launch_key_permute(const KernelEnv &env, const u64 *src, u64 *dst, const uint32_t *perm, u64 n_polys);
// out [n_ops][2][L][N] = sigma_g(in.c0 + u.0, u.1), NTT form, perm = the element's NTT-domain permutation; plain ([L][N], optional):
// out = plain (.) that (first) or out += plain (.) that
void launch_hoist_finish_ntt(const KernelEnv &env, int L, u64 n_ops, const u64 *u, const u64 *in, const uint32_t *perm, u64 *out, const u64 *plain = nullptr,
                             bool first = true);
// One term of the lazy plain sum (he355_rotate_hoisted_plain_sum_lazy), plain_qp [L + 1][N] with row L under the special prime.
// Keyed (t not null): t [n_ops][2][L][N] / tpr [n_ops][2][N] as launch_k3(K3_ALL) leaves them under the element's permuted key ->
// A += plain_qp (.) sigma(t, NTT(tpr)), A = (aq: n_ops x aq_op_stride, [2][L][N] each; ap [n_ops][2][N], canonical NTT form under the
// special prime), and out[.][0] += plain_qp (.) sigma(in.c0).  The identity (t null): out += plain_qp (.) in, both polynomials.
// first_a / first_b: the accumulator A / out starts with this term (stored, not read; a keyed first term zeroes out[.][1]).
void launch_hoist_acc_qp(const KernelEnv &env, int L, u64 n_ops, const u64 *t, const u64 *tpr, const u64 *in, const uint32_t *perm, const u64 *plain_qp, u64 *aq,
                         u64 aq_op_stride, u64 *ap, u64 *out, bool first_a, bool first_b);
// The baby-step/giant-step transform (he355_linear_transform_bsgs).  The rotate kernel: t / tpr as launch_k3(K3_ALL) leaves them under the
// element's permuted key, `in` [n_ops][2][L][N] the ciphertexts whose c1 was switched -> sigma(t + P in.c0, t.1) under the data primes into
// dq + (op * 2 + k) * dq_poly_stride + i * N, sigma(NTT(tpr)) into dp + (op * 2 + k) * dp_poly_stride; acc: added into what lies there.
void launch_hoist_rot_qp(const KernelEnv &env, int L, u64 n_ops, const u64 *t, const u64 *tpr, const u64 *in, const uint32_t *perm, u64 *dq, u64 dq_poly_stride, u64 *dp,
                         u64 dp_poly_stride, bool acc);
// the identity baby: dst [n_ops][2][L + 1][N] = P (.) in under the data primes, 0 under the special prime
void launch_bsgs_ident(const KernelEnv &env, int L, u64 n_ops, const u64 *in, u64 *dst);
// one giant row's inner sum: store [slots][n_ops][2][L + 1][N], plain_row = the row's plaintexts ([L + 1][N] each), terms [n_terms] device
// pairs (slot, plaintext of the row) -> dq [n_ops][2][L][N], dp [n_ops][2][N]; acc: added into what lies there
void launch_bsgs_inner(const KernelEnv &env, int L, u64 n_ops, const u64 *store, const u64 *plain_row, const uint32_t *terms, u64 n_terms, u64 *dq, u64 *dp, bool acc);
// he355_combine_scalars (he355_kernels_poly.hip): out [n][size][L][N] = sum_t scalars[t][i] * term_t + (polynomial 0: cst[i]); d_terms [n_terms]
// device pairs of words {the term's slab [n][size][L_t][N], L_t >= L}, d_scalars [n_terms][L], d_const [L] or null -- all canonical
void launch_scalar_combine(const KernelEnv &env, int L, int size, u64 n, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const, u64 *out);
// he355_combine_scalars_rescale (he355_kernels_cheb.hip; arithmetic: cheb_core.h): the same tables as launch_scalar_combine, read from ciphertext
// op_off of the terms' slabs on.  Row L - 1 of the combination alone -> row [n size][N]; then, behind the inverse row pass of `row` and
// launch_floor_cols(prime L - 1 -> L - 1 targets) into cols [n size][L - 1][N], out [n][size][L - 1][N] = (combination - NTT(cols)) * q_(L-1)^-1
void launch_scalar_combine_row(const KernelEnv &env, int L, int size, u64 n, u64 op_off, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const, u64 *row);
void launch_floor_rows_combine(const KernelEnv &env, int L, int size, u64 n, u64 op_off, const u64 *cols, const void *d_terms, u64 n_terms, const u64 *d_scalars,
                               const u64 *d_const, u64 *out);
// ---- complex CKKS slots (he355_kernels_cplx.hip; arithmetic: cplx_core.h) --------------------------------------------------------------------
// he355_combine_scalars_complex: launch_scalar_combine with d_scalars [n_terms][2][L] and d_const [2][L] or null, the half picked by bit
// (log2 N - 2) of the NTT index
void launch_scalar_combine_cplx(const KernelEnv &env, int L, int size, u64 n, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const, u64 *out);
// values [n][count][2] (re, im) -> plain [n][Ltop][N] coefficient form, as launch_ckks_encode
void launch_ckks_encode_cplx(const KernelEnv &env, u64 n_vec, const double *values, u64 count, double scale, void *zbuf, u64 *plain, const EncTablesDev &t, int *err);
// zbuf [n][N] as launch_ckks_decode leaves it (the finished transforms) -> out [n][sr.total][2]: (re, im) of the slots of sr's ranges
void launch_ckks_gather_cplx(const KernelEnv &env, u64 n_vec, const void *zbuf, double *out, const EncTablesDev &t, const SlotRanges &sr);
// ---- the CKKS modulus raise (he355_kernels_raise.hip; arithmetic: raise_core.h) ------------------------------------------------------------
// coeff [n_polys][N], coefficients canonical under q_0 -> rows first .. L_to - 1 of out [n_polys][L_to][N]: the centred coefficient mod q_j,
// canonical, coefficient form (first = 0: he355_ckks_lift_centred; first = 1: row 0 is the caller's).  One streaming launch.
void launch_raise_lift(const KernelEnv &env, int L_to, int first, u64 n_polys, const u64 *coeff, u64 *out);
// tail [n_polys][N] as launch_rows_inv_select(prime 0) leaves it -> rows 1 .. L_to - 1 of out [n_polys][L_to][N] after the forward column pass
// (raw of prime j; launch_rows_fwd finishes them in place).  tsplit > 1: a column's targets dealt to that many blocks.  N >= 2048 only.
void launch_raise_cols(const KernelEnv &env, int L_to, u64 n_polys, const u64 *tail, u64 *out, int tsplit = 1);
// he355_plain_extend_special's streaming half: src [n][L][N] NTT form -> dst [n][L + 1][N], rows 0 .. L - 1 copied, row L = the coefficients
// of row 0 (coeff [n][Lc][N], coefficient form) centred and reduced mod the special prime, coefficient form (launch_ntt_forward follows).
// mismatch (optional, one device word, zeroed by the caller; needs Lc = L, else Lc = 1): += the (coefficient, prime >= 1) pairs that disagree
void launch_plain_extend(const KernelEnv &env, int L, u64 n, const u64 *src, const u64 *coeff, int Lc, u64 *dst, u64 *mismatch);
// dst [n_ops][2][L][N] = (ct.c0, 0)
void launch_hoist_addend_coeff(const KernelEnv &env, int L, u64 n_ops, const u64 *ct, u64 *dst);
// out [n_ops][2][L][N] = the signed coefficient gather of src, both polynomials
void launch_hoist_finish_coeff(const KernelEnv &env, int L, u64 n_ops, const u64 *src, const uint32_t *gather, u64 *out);
// inverse row pass of one residue of each poly: src [(op,k)] residue `prime` -> tail [(op,k)][N]
void launch_rows_inv_select(const KernelEnv &env, int prime, u64 n_polys, const u64 *src, u64 src_poly_stride, u64 *tail);
// ---- client side on the device: encryption / decryption (SURVEY.md 8f rank 1) ------------------------------
// u [n][K][N], e [n][2][K][N]: sampled polynomials of ciphertexts first_index.. (coefficient form, canonical residues)
void launch_enc_sample(const KernelEnv &env, u64 n_cts, u64 seed, u64 first_index, u64 *u, u64 *e);
// z[r][k][i] = u[r][i] (.) pk[k][i] (+ z if add_in); NTT form at the key level
void launch_enc_mul_pk(const KernelEnv &env, u64 n_cts, const u64 *u, const u64 *pk, u64 *z, bool add_in);
// coefficient-form divide-and-round by the special prime: z [n_polys][K][N] -> out [n_polys][K-1][N]
void launch_divround_last_coeff(const KernelEnv &env, u64 n_polys, const u64 *z, u64 *out);
void launch_dot_sk(const KernelEnv &env, int L, int size, u64 n_cts, const u64 *ct, const u64 *sk, u64 *out);
void launch_bfv_scale_round(const KernelEnv &env, u64 n_cts, const u64 *phase, u64 *plain, const CrtTablesDev &c);
// values [n][count] -> plain [n][Ltop][N] coefficient form (zbuf: [n][N] complex scratch; *err |= 1 if a coefficient overflows)
void launch_ckks_encode(const KernelEnv &env, u64 n_vec, const double *values, u64 count, double scale, void *zbuf, u64 *plain, const EncTablesDev &t, int *err);
// coeff [n][L][N] coefficient form -> out [n][sr.total]: the slots of sr's ranges, concatenated
void launch_ckks_decode(const KernelEnv &env, u64 n_vec, const u64 *coeff, double scale, void *zbuf, double *out, const EncTablesDev &t, const CrtTablesDev &c,
                        const SlotRanges &sr);
void launch_bfv_encode_scatter(const KernelEnv &env, u64 n_vec, const long long *values, u64 count, u64 *ev, const uint32_t *slot_index, u64 t);
void launch_bfv_decode_gather(const KernelEnv &env, u64 n_vec, const u64 *ev, long long *out, const uint32_t *slot_index, u64 t, const SlotRanges &sr);
// ---- key generation on the device --------------------------------------------------------------------------------
// key [Ltop][2][K][N] <- key-switching key for new_key = s^2 (perm == null) or s permuted by `perm` (Galois key);
// e_scratch [Ltop][K][N], target_scratch [K][N]; randomness: keygen_stream(key_id, digit, ...) of client/sampler.h, the uniform halves from
// `a_seed` and the errors from `noise_seed` (one seed for both: the keys of he355_keygen_relin / he355_keygen_galois)
void launch_keygen_kswitch(const KernelEnv &env, u64 *key, u64 *e_scratch, u64 *target_scratch, const u64 *sk, const uint32_t *perm, u64 a_seed, u64 noise_seed, u64 key_id);
// ---- key switch with one workgroup per residue polynomial, transforms resident in LDS (N <= 8192; he355_kernels_lds.hip) ----------
// out[op] (out_op_stride words apart, [2][L][N]) = addend + key switch of the target under `key`; part: scratch of n_ops * ks_lds_part_words words
bool ks_lds_supported(const KernelEnv &env, int L);
u64 ks_lds_part_words(const KernelEnv &env, int L);
void launch_ks_lds(const KernelEnv &env, int L, u64 n_ops, const LdsKsOperands &src, const u64 *key, u64 *part, u64 *out, u64 out_op_stride);
// CKKS rescale in the same shape: src [size][L][N] per op -> out [n_ops][size][L - 1][N], one launch
void launch_rescale_lds(const KernelEnv &env, int L, int size, u64 n_ops, const u64 *src, u64 src_op_stride, u64 *out);
// ---- BFV level operations on coefficient-form ciphertexts (he355_kernels_bfv_level.hip; arithmetic: bfv_level_core.h) -------------------
// Evaluator::mod_switch_to for BFV: in [n_polys][L][N] -> out [n_polys][L_to][N], the L - L_to divide-and-round steps in one launch.
// tab: device copy of bfv_drop_table, entry [j * stride + i].  L <= kBfvLevelMaxL.
void launch_bfv_mod_switch(const KernelEnv &env, const BfvDropConst *tab, int stride, int L, int L_to, u64 n_polys, const u64 *in, u64 *out);
// out[r] = ct[ia(r)] +- (Delta_L(plain[ib(r)]), 0, ..); plain [.][N] mod t.  out may be ct where every ciphertext serves one result
// (he355_encrypt: the plaintext term at the top level, pairwise, in place)
void launch_bfv_addsub_plain(const KernelEnv &env, int L, int size, u64 n_results, const u64 *ct, const u64 *plain, Indexer ix, u64 *out, const BfvDeltaConst &dc,
                             bool sub);
// multiply_plain: plain [n_plain][N] mod t -> dst [n_plain][L][N] centred lift (coefficient form; launch_ntt_forward then prepares it);
// forward column pass ct[ia(r)] -> out[r] (nothing when N = 1024); forward row pass x prepared plaintext row, inverse row pass, in place
// on out (N = 1024: ct -> out) -- launch_cols_inv finishes.  r = op_offset .. op_offset + n_ops - 1; ct, prep, out: the batch's pointers
void launch_bfv_lift_plain(const KernelEnv &env, int L, u64 n_plain, const u64 *plain, u64 *dst, u64 t);
void launch_bfv_mp_cols_fwd(const KernelEnv &env, int L, int size, u64 n_ops, u64 op_offset, const u64 *ct, Indexer ix, u64 *out);
void launch_bfv_mp_rows(const KernelEnv &env, int L, int size, u64 n_ops, u64 op_offset, const u64 *ct, const u64 *prep, Indexer ix, u64 *out);
// ---- BFV invariant noise budget (he355_kernels_bfv_noise.hip; arithmetic: bfv_noise_core.h) ----------------------------------------------
// ct [n_cts][size][L][N] -> tmp [n_cts][size - 1][L][N]: polynomials 1 .. size-1, the ones the phase needs transformed
void launch_bfv_noise_take(const KernelEnv &env, int L, int size, u64 n_cts, const u64 *ct, u64 *tmp);
// tmp in NTT form -> out [n_cts][L][N] = (c_{size-1} s + .. + c_1) s, NTT form
void launch_bfv_noise_dot_sk(const KernelEnv &env, int L, int size, u64 n_cts, const u64 *tmp, const u64 *sk, u64 *out);
// bits[r] = max(bits[r], bit length of the largest centred coefficient of t (part[r] + ct[r][0]) mod q_L); part [n_cts][L][N] coefficient form
void launch_bfv_noise_bits(const KernelEnv &env, int size, u64 n_cts, const u64 *part, const u64 *ct, int *bits, const CrtTablesDev &crt, const BfvNoiseConst &c);
// in place: budget[r] = max(0, q_bits - budget[r] - 1); noise_bits[r] (if given) = the value that came in
void launch_bfv_noise_finish(const KernelEnv &env, u64 n_cts, int *budget, int *noise_bits, int q_bits);
// ---- NTT-form BFV plaintext inner product (he355_kernels_bfv_ntt.hip; arithmetic: bfv_mac_core.h) ---------------------------------------------
// out(i, j) = sum_k ct(i, k) (.) pt(k, j), canonical residues: ct [.][size][L][N] and pt [.][L][N] in NTT form, ciphertext (i, k) at index
// i * ct_stride_i + k * ct_stride_k, plaintext (k, j) at k * pt_stride_k + j * pt_stride_j; out [rows * cols][size][L][N].  One launch.
void launch_bfv_plain_mac(const KernelEnv &env, int L, int size, u64 rows, u64 cols, u64 inner, const u64 *ct, u64 ct_stride_i, u64 ct_stride_k, const u64 *pt,
                          u64 pt_stride_k, u64 pt_stride_j, u64 *out);
// ---- BFV monomial multiply and the odd children of he355_bfv_expand (he355_kernels_bfv_expand.hip; arithmetic: bfv_expand_core.h) -----------
// out[p] = x[p] X^e in Z_q[X]/(X^N + 1), e in [0, 2N), for n_polys residue polynomials [.][L][N] in coefficient form (polynomial p under
// prime p % L): x = in, or (even != null) 2 in - even -- the odd child X^(-s) (c - g) of the expansion from the node c and its even child
// c + g.  out may overlap neither operand.  One launch.
void launch_bfv_shift(const KernelEnv &env, int L, u64 n_polys, const u64 *in, const u64 *even, u32 e, u64 *out);
// one level of he355_bfv_merge (arithmetic: bfv_merge_core.h): pair p = k n + r, k < s = 2^j, r < n, has its even operand at ciphertext
// k stride_k + r stride_r of `in` ([2][L][N] words each) and its odd operand s stride_k behind it; S[p] = even + X^s odd, D[p] = even - X^s odd,
// and S[p] = D[p] = even for the pairs p >= full, whose partner is absent.  S and D may overlap neither each other nor an operand.  One launch.
void launch_bfv_merge(const KernelEnv &env, int L, u64 n, u64 s, u64 full, const u64 *in, u64 stride_k, u64 stride_r, u64 *S, u64 *D);
// ---- BFV ciphertext decomposition for recursive PIR (he355_kernels_bfv_digits.hip; arithmetic: bfv_digits_core.h) ---------------------------
// ct [n][size][L][N] coefficient form <-> plain [n][F][N] mod t, F = size D(L): digit g of polynomial k under prime i is plaintext
// k D(L) + off_i + g (`tab`: bfv_digit_table of the level).  One launch each; the two slabs may not overlap.
void launch_bfv_digits(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *ct, u64 *plain);
void launch_bfv_undigits(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *plain, u64 *ct);
// The forward column pass of the digits' transforms, out of place: ct -> out [n][F][L_out][N], the centred lift of digit plaintext f under
// prime i' < L_out after the column pass (raw of prime i'), what launch_bfv_lift_plain + launch_cols_fwd would have left there;
// launch_rows_fwd finishes it in place.  N >= 2048 only (N = 1024 has no column pass).
void launch_bfv_digits_cols_fwd(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *ct, int L_out, u64 t, u64 *out);
// ---- a PIR database from packed bytes (he355_kernels_bfv_bytes.hip; arithmetic: bfv_bytes_core.h) --------------------------------------------
// Plaintext j is the B bytes at bytes + j stride read as one little-endian integer, coefficient e its bits [e w, e w + w).  `bytes` of
// launch_bfv_unpack / launch_bfv_bytes_cols_fwd is any byte address and stride any value >= B: only aligned 8-byte words that hold a valid
// byte of the plaintext at hand are read.  plain [n][N] coefficients mod t.  One launch each; the two sides may not overlap.
void launch_bfv_unpack(const KernelEnv &env, int w, u64 n, const void *bytes, u64 stride, u64 B, u64 *plain);
// the inverse: ceil(B / 8) whole words per plaintext, the bytes past B in the last one zero; `bytes` 8-byte aligned, stride a multiple of 8
// and at least 8 ceil(B / 8); every input word is masked to w bits
void launch_bfv_pack(const KernelEnv &env, int w, u64 n, const u64 *plain, u64 B, u64 stride, void *bytes);
// The forward column pass of the plaintexts' transforms, out of place: bytes -> out [n][L_out][N], the centred lift of plaintext j under
// prime i' < L_out after the column pass (raw of prime i'), what launch_bfv_unpack + launch_bfv_lift_plain + launch_cols_fwd would have left
// there; launch_rows_fwd finishes it in place.  N >= 2048 only (N = 1024 has no column pass).
void launch_bfv_bytes_cols_fwd(const KernelEnv &env, int w, u64 n, const void *bytes, u64 stride, u64 B, int L_out, u64 t, u64 *out);
// ---- BFV reply compression (he355_kernels_bfv_reply.hip; arithmetic: bfv_reply_core.h) ------------------------------------------------------
// Reply j is the N (k0 + k1) / 64 words at bytes + j stride (`bytes` 8-byte aligned, stride a multiple of 8 that holds a reply): c0's N
// fields of k0 bits, then c1's N fields of k1 bits, under q_0 = env.prime_q[0].  ct [n][2][N], L = 1, coefficient form.
void launch_bfv_reply_pack(const KernelEnv &env, int k0, int k1, u64 n, const u64 *ct, u64 stride, void *bytes);
// out [n][N]: c1's fields centred and lifted mod q_0
void launch_bfv_reply_lift(const KernelEnv &env, int k0, int k1, u64 n, const void *bytes, u64 stride, u64 *out);
// prod [n][N]: the negacyclic product of the lifted c1 and the secret key mod q_0 -> plain [n][N] mod t; bits [n] (or null: nothing is
// gathered): the maximum of the residues' bit lengths is atomicMax'ed into it, zeroed by the caller on the same stream
void launch_bfv_reply_finish(const KernelEnv &env, int k0, int k1, u64 t, u64 n, const void *bytes, u64 stride, const u64 *prod, u64 *plain, int *bits);
// ---- the BFV external product RGSW x ciphertext (he355_kernels_bfv_gadget.hip; arithmetic: bfv_gadget_core.h, bfv_mac_core.h) ----------------
// The gadget cut in NTT form: ciphertext (a, b), a < n_a, b < n_b, at index a stride_a + b stride_b of `ct` ([size][L][N], coefficient
// form) -> out [(a n_b + b) size E + f][L][N], digit polynomial f = k E(L) + off_i + g under every prime j < L (`tab`: bfv_gadget_table of the
// level).  cols (N >= 2048 only): the forward column pass (raw columns; launch_rows_fwd finishes in place).  Else: the digits in coefficient
// form (launch_ntt_forward follows in place).
void launch_bfv_gadget_cut(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n_a, u64 n_b, const u64 *ct, u64 stride_a, u64 stride_b, u64 *out, bool cols);
// out[r] = sum_(kappa < inner) sum_(f < rows) dig[r][kappa][f] (.) row f of RGSW (r, kappa), both polynomials, canonical NTT form: dig
// [n][inner][rows][L][N], RGSW (r, kappa) at index r rg_stride_r + kappa rg_stride_k of `rgsw`, [rows][2][L][N] each; out [n][2][L][N].
void launch_bfv_gadget_mac(const KernelEnv &env, int L, u64 n, u64 inner, u32 rows, const u64 *dig, const u64 *rgsw, u64 rg_stride_r, u64 rg_stride_k, u64 *out);
// zero [n 2E][2][L_in][N] encryptions of zero (coefficient form, L_in >= L), plain [n][N] mod t -> out [n 2E][2][L][N]: the first L primes of
// each row plus lift(m) 2^(g v) mod q_i in polynomial k under prime i of row k E + off_i + g.  In place (out == zero) when L_in == L.
void launch_bfv_rgsw_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, int L_in, u64 n, const u64 *zero, const u64 *plain, u64 t, u64 *out);
// ---- RGSW selectors from one packed query ciphertext (he355_kernels_bfv_gadget.hip; arithmetic: bfv_gadget_core.h) -------------------------------
// launch_bfv_gadget_cut for he355_bfv_rgsw_from_bfv: slot ciphertexts first .. first + count - 1 of the order c = a n_b + b (ciphertext c at
// index a stride_a + b stride_b of `ct`, [2][L][N]) -> out [count][2 E_key][L][N] (`tab`: the key's table), and ciphertext c itself, transformed as
// the digits are (cols: its raw column; else coefficient form), into row bfv_selector_row(c, own_E, 0) of own [.][2 own_E][2][L][N].
void launch_bfv_gadget_cut_own(const KernelEnv &env, const BfvDigitTab &tab, int L, u64 n_b, u64 first, u64 count, const u64 *ct, u64 stride_a, u64 stride_b, u64 *out,
                               u64 *own, u32 own_E, bool cols);
// row bfv_selector_row(first + r, own_E, 1) of out = sum_(f < rows) dig[r][f] (.) row f of `key` ([rows][2][L][N]), r < count, canonical NTT form
void launch_bfv_gadget_mac_own(const KernelEnv &env, int L, u64 first, u64 count, u32 rows, const u64 *dig, const u64 *key, u64 *out, u32 own_E);
// zero [n][2][L_in][N] encryptions of zero (coefficient form, L_in >= L), sel [n][n_sel] mod t -> out [n][2][L][N]: the first L primes plus
// bfv_selector_value of selector b, digit (i, g), at coefficient first_slot + b E + off_i + g of polynomial 0 under prime i; d = the expansion's
// depth.  In place (out == zero) when L_in == L.
void launch_bfv_selector_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, int L_in, u64 n, u64 n_sel, u64 first_slot, int d, const u64 *zero, const u64 *sel, u64 t, u64 *out);
// s [N]: the secret key's coefficients under prime 0 (0, 1, q_0 - 1), in place -> mod t (0, 1, t - 1)
void launch_bfv_secret_plain(const KernelEnv &env, u64 *s, u64 t);
// ---- the BFV selection tree (he355_bfv_select; he355_kernels_bfv_gadget.hip; arithmetic: bfv_gadget_core.h) --------------------------------------
// One pass of one level.  Pair c = first + (index in the pass) of the level is (r, b) = (c / group, c % group), group = the pairs per result; its
// even node is the ciphertext ([2][L][N], coefficient form) at index r stride_a + 2 b stride_b of `nodes`, its odd node stride_b behind it.
// The cut of odd - even into out [count][2E][L][N], as launch_bfv_gadget_cut (cols: raw columns, launch_rows_fwd finishes; else coefficient form)
void launch_bfv_select_cut(const KernelEnv &env, const BfvDigitTab &tab, int L, u64 group, u64 first, u64 count, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out, bool cols);
// out[pair] = sum_(f < rows) dig[pair][f] (.) row f of the RGSW ciphertext at index r rg_stride_r of `rgsw`, canonical NTT form, out [count][2][L][N]
void launch_bfv_select_mac(const KernelEnv &env, int L, u64 group, u64 first, u64 count, u32 rows, const u64 *dig, const u64 *rgsw, u64 rg_stride_r, u64 *out);
// node (r, b) of the next level, the ciphertext at index r out_stride + b of `out`, = even node + sums[pair].  N >= 2048: sums are the raw rows
// launch_rows_inv leaves, and the launch is the inverse column pass with the add behind it; N = 1024: sums are coefficients, a streaming add
void launch_bfv_select_tail(const KernelEnv &env, int L, u64 group, u64 first, u64 count, const u64 *sums, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out, u64 out_stride);
// node 2 group of every result r < n (the one without a partner) -> node `group` of the next level; group = 0: a level of one node
void launch_bfv_select_copy(const KernelEnv &env, int L, u64 n, u64 group, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out, u64 out_stride);
// ---- seeded BFV queries and Galois keys (he355_kernels_bfv_seeded.hip; arithmetic: bfv_seeded_core.h) ---------------------------------------------
// The uniform polynomials a seed stands for, NTT form: polynomial (item, i), item < items, i < polys, is
// sample_uniform_at(seed, stream0 + item stream_step + i, ., q_i), written to out + item item_stride + i N.  sk ([.][N] NTT form, row i under
// prime i) not null: its product with row i of sk is written instead.  One launch.
void launch_bfv_seeded_gen(const KernelEnv &env, int polys, u64 items, u64 seed, u64 stream0, u64 stream_step, u64 *out, u64 item_stride, const u64 *sk);
// w [n][L][N] = iNTT(a (.) s), plain [n][N] mod t (null: zeros) -> c0 [n][L][N] = Delta_L(m) - e - w, e = sample_cbd_at(noise_seed,
// seeded_e_stream(first_index + r), .); c0 may be w
void launch_bfv_seeded_finish(const KernelEnv &env, int L, u64 n, const u64 *w, const u64 *plain, const BfvDeltaConst &dc, u64 noise_seed, u64 first_index, u64 *c0);
// c0 [n][L][N] -> polynomial 0 of out [n][2][L][N]
void launch_bfv_seeded_place(const KernelEnv &env, int L, u64 n, const u64 *c0, u64 *out);
// launch_bfv_selector_plant's plant, added in place to c0 [n][L][N]
void launch_bfv_seeded_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, u64 n, u64 n_sel, u64 first_slot, int d, const u64 *sel, u64 t, u64 *c0);
