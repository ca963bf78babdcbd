// Host build of the ct x ct prologue of k_k3<TENSOR> (csrc/modarith.h: dy_mul3) and of the sums it starts, for
// tests/test_tensor_prologue_cpu.py: c0, c1, c2 from the four operand residues, then `terms` further key products into the c1 sum the way
// the kernel's digit loop adds them, for both engines.  Compiled by the test, once per form of the u64 engine (-DHE355_U64_FOLD=0 / 1),
// and loaded through ctypes.
#include <cstddef>

#include "modarith.h"

using namespace he355;

namespace {
ArF64 make_f64(u64 q)
{
    ArF64 a;
    a.q = (double)q;
    a.qinv = 1.0 / (double)q;
    a.ninv = 0;
    a.ninv_i = 0;
    return a;
}
ArU64 make_u64(u64 q)
{
    ArU64 a;
    a.q = q;
    a.two_q = 2 * q;
    a.ninv = a.ninv_q = 0;
    const u128 c = ~(u128)0 / q; // floor(2^128 / q): q is odd, so 2^128 - 1 has the same quotient
    a.cr0 = (u64)c;
    a.cr1 = (u64)(c >> 64);
    return a;
}
} // namespace

extern "C" {
int tp_fold_build() { return HE355_U64_FOLD; }
unsigned tp_tensor_terms() { return kTensorTerms; }
unsigned tp_direct_terms(u64 q) { return floor_direct_terms(q); }
int tp_direct(unsigned acc_terms, unsigned terms) { return floor_direct(acc_terms, terms) ? 1 : 0; }
double tp_term_bound(u64 q) { return floor_term_bound(q); }
double tp_acc_max() { return kFloorAccMax; }
int tp_acc_run() { return ArU64::kAccRun; }

// fp64 engine.  c0, c1, c2: the doubles as the kernel holds them (centred lazy).  sum1: c1 and then, per element, the `terms` products
// x[j] * key[j] (x: a transformed digit as a double, any integer inside the key product's range; key: canonical), as acc_mac adds them.
// s2 = the prime a rescale divides by: fin2[i] = floor_fin2_s_acc(sum1, corr[i]), the headline's floor step, read from the sum as it is.
void tp_f64(u64 q, u64 s2, size_t n, const u64 *a0, const u64 *a1, const u64 *b0, const u64 *b1, int terms, const double *x, const u64 *key,
            const double *corr, double *c0, double *c1, double *c2, double *sum1, u64 *fin2)
{
    const ArF64 ar = make_f64(q);
    struct { double inv_d, inv_i; } f2;
    u64 inv = 1, b = s2 % q, e = q - 2;
    while (e) {
        if (e & 1) inv = (u64)((u128)inv * b % q);
        b = (u64)((u128)b * b % q);
        e >>= 1;
    }
    f2.inv_d = (double)inv;
    f2.inv_i = (double)inv / (double)q;
    for (size_t i = 0; i < n; ++i) {
        ar.dy_mul3(ar.dy_in(a0[i]), ar.dy_in(a1[i]), ar.dy_in(b0[i]), ar.dy_in(b1[i]), c0[i], c1[i], c2[i]);
        ArF64::Acc acc = ar.acc_from_lazy(c1[i]);
        for (int j = 0; j < terms; ++j) ar.acc_mac(acc, x[j], ar.key_in(ar.to_raw((double)key[j])), 0);
        sum1[i] = acc;
        fin2[i] = ar.floor_fin2_s_acc(acc, corr[i], f2);
    }
}

// u64 engine.  c0, c1, c2 canonical; sum1: c1 and `terms` products x[j] * key[j] (x any lazy value below 4q), added in runs of kAccRun
// between two acc_reduce as k_k3 does, and brought to the canonical residue by acc_canon.  overflow: a lazy run wrapped (it may not).
void tp_u64(u64 q, size_t n, const u64 *a0, const u64 *a1, const u64 *b0, const u64 *b1, int terms, const u64 *x, const u64 *key, u64 *c0, u64 *c1,
            u64 *c2, u64 *sum1, int *overflow)
{
    const ArU64 ar = make_u64(q);
    *overflow = 0;
    for (size_t i = 0; i < n; ++i) {
        ar.dy_mul3(ar.dy_in(a0[i]), ar.dy_in(a1[i]), ar.dy_in(b0[i]), ar.dy_in(b1[i]), c0[i], c1[i], c2[i]);
        ArU64::Acc acc = ar.acc_from_lazy(c1[i]);
        int pend = 0;
        for (int j = 0; j < terms; ++j) {
            const u64 k2 = pre_word(key[j], q, HE355_U64_FOLD != 0);
            const u64 before = acc;
            ar.acc_mac_lazy(acc, x[j], key[j], k2);
            if (acc < before) *overflow = 1;
            if (++pend == ArU64::kAccRun) {
                acc = ar.acc_reduce(acc);
                pend = 0;
            }
        }
        if (pend) acc = ar.acc_reduce(acc);
        sum1[i] = ar.acc_canon(acc);
    }
}
}
