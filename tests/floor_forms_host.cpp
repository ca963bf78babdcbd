// Host build of the floor steps of csrc/modarith.h for tests/test_floor_forms_cpu.py: the composition k_k3's epilogue used to write
// (floor_fin*(acc_canon(acc), ...)) and the forms that take the accumulator, over arrays, for both engines.  Compiled by the test,
// once per form of the u64 engine (-DHE355_U64_FOLD=0 / 1), and loaded through ctypes.
#include <cstddef>

#include "device_tables.h"
#include "modarith.h"

using namespace he355;

namespace {
// the floor steps' constants are the product's own: floor_const of csrc/device_tables.h, as DeviceContext::init uploads them
using FC = FloorConst;
FC make_fc(u64 qs, u64 qi) { return floor_const(qs, qi, HE355_U64_FOLD != 0); }
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
    // floor(2^128 / q) as two words (q is odd, so 2^128 - 1 has the same quotient)
    const u128 all = ~(u128)0;
    const u128 c = all / q;
    a.cr0 = (u64)c;
    a.cr1 = (u64)(c >> 64);
    return a;
}
// form: 0 floor_fin, 1 floor_fin2, 2 floor_fin_s, 3 floor_fin2_s.  mode: 0 the old composition, 1 the accumulator form as it is (operands
// inside the form's range), 2 the accumulator form behind floor_prep (what a launch beyond the host-side bound runs)
template <class Ar, class A, class X>
void run(const Ar &ar, int form, int mode, const FC &f1, const FC &f2, size_t n, const A *acc, const X *x, const u64 *addend, u64 *out)
{
    for (size_t i = 0; i < n; ++i) {
        u64 r;
        if (mode == 0) {
            const u64 t = ar.acc_canon(acc[i]);
            r = form == 0   ? ar.floor_fin(t, x[i], f1.inv, f1.inv_shoup, f1.inv_d, f1.inv_i, addend[i])
                : form == 1 ? ar.floor_fin2(t, x[i], f1, f2, addend[i])
                : form == 2 ? ar.floor_fin_s(t, x[i], f1.inv, f1.inv_shoup, f1.inv_d, f1.inv_i)
                            : ar.floor_fin2_s(t, x[i], f2);
        } else {
            typename Ar::Acc a = acc[i];
            typename Ar::T y = x[i];
            if (mode == 2) ar.floor_prep(a, y);
            r = form == 0   ? ar.floor_fin_acc(a, y, f1.inv, f1.inv_shoup, f1.inv_d, f1.inv_i, addend[i])
                : form == 1 ? ar.floor_fin2_acc(a, y, f1, f2, addend[i])
                : form == 2 ? ar.floor_fin_s_acc(a, y, f1.inv, f1.inv_shoup, f1.inv_d, f1.inv_i)
                            : ar.floor_fin2_s_acc(a, y, f2);
        }
        out[i] = r;
    }
}
} // namespace

extern "C" {
int ff_fold_build() { return HE355_U64_FOLD; }
// s1^-1 and s2^-1 mod q as the two steps' constants (s1: the special prime, s2: the prime the rescale divides by); the inverses come back
// through inv[0], inv[1] so that the caller's integers use the same constants
void ff_f64(u64 q, u64 s1, u64 s2, int form, int mode, size_t n, const double *acc, const double *x, const u64 *addend, u64 *out, u64 *inv)
{
    const FC f1 = make_fc(s1, q), f2 = make_fc(s2, q);
    inv[0] = f1.inv;
    inv[1] = f2.inv;
    run(make_f64(q), form, mode, f1, f2, n, acc, x, addend, out);
}
void ff_u64(u64 q, u64 s1, u64 s2, int form, int mode, size_t n, const u64 *acc, const u64 *x, const u64 *addend, u64 *out, u64 *inv)
{
    const FC f1 = make_fc(s1, q), f2 = make_fc(s2, q);
    inv[0] = f1.inv;
    inv[1] = f2.inv;
    run(make_u64(q), form, mode, f1, f2, n, acc, x, addend, out);
}
// the raw tail's forms: what reaches the inverse row pass from a sum, directly and through the parked word; as canonical residues
// (to_canon) and as the magnitude bound the engine promises (fp64 engine: |x| <= q/2 + 1 -> ok[i] = 1)
void ff_f64_to_inv(u64 q, size_t n, const double *acc, u64 *direct, u64 *parked, unsigned char *ok)
{
    const ArF64 ar = make_f64(q);
    for (size_t i = 0; i < n; ++i) {
        const double a = ar.acc_to_inv(acc[i]), b = ar.acc_unpark(ar.acc_park(acc[i]));
        direct[i] = ar.to_canon(a);
        parked[i] = ar.to_canon(b);
        const double lim = 0.5 * (double)q + 1.0;
        ok[i] = (a <= lim && a >= -lim && a == b) ? 1 : 0;
    }
}
// the host-side selection (PrimeDev::acc_terms and what the kernel evaluates against it)
u32 ff_direct_terms(u64 q) { return floor_direct_terms(q); }
double ff_term_bound(u64 q) { return floor_term_bound(q); }
double ff_x_bound(u64 q) { return f64_stage_growth(4.0 * (double)q, (double)q, 15); }
int ff_direct(u32 acc_terms, u32 terms) { return floor_direct(acc_terms, terms) ? 1 : 0; }
double ff_acc_max() { return kFloorAccMax; }
double ff_x_max() { return kFloorXMax; }
}
