// he355_api.hip — the device context (the engine: memory, keys, chunk loop, key switch, rotations, BFV multiply, client calls) and the C ABI
// declared in include/he355.h; four call families have their launch sequences with their entry points in the .inc files included last.
// Host code is C++17; the only way into the GPU is through the launchers of he355_kernels.h.
// There is no CPU implementation of any evaluator op in this library: without a HIP device every device
// entry point fails with HE355_E_DEVICE.
#include <hip/hip_runtime.h>

#include <array>
#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/he355.h"
#include "behz_lists.h"
#include "bfv_pir_args.h"
#include "device_pool.h"
#include "device_tables.h"
#include "he355_internal.h"
#include "he355_kernels.h"
#include "he_params.h"
#include "hoist_args.h"
#include "ntt_core.h"
#include "poly_args.h"
#include "cheb_args.h"
#include "raise_args.h"
#include "rotation_plan.h"
#include "client/he_client.h"
#include "client/multiword.h"

namespace he355 {

#define HIPCHECK(expr)                                                                                             \
    do {                                                                                                           \
        hipError_t e__ = (expr);                                                                                   \
        if (e__ != hipSuccess)                                                                                     \
            throw DeviceError(std::string("HIP error: ") + hipGetErrorString(e__) + " in " #expr " (" __FILE__ ":" + \
                              std::to_string(__LINE__) + ")");                                                     \
    } while (0)

namespace {

__device__ __forceinline__ u64 splitmix64(u64 x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct PrimeMap {
    unsigned char prime_of[64];
    u32 period;
};

// uniform-looking residues in [0, q): counter-based generator, value = floor(rand64 * q / 2^64)
// first_poly: index of dst's first polynomial in the whole (virtual) array the stream belongs to -- a shard of a batch filled with
// its offset holds exactly the values the full batch would hold there, whatever the number of shards
__global__ void k_fill_uniform(u64 *dst, u64 n_polys, int logN, const PrimeDev *primes, PrimeMap pm, u64 seed, u64 first_poly)
{
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 poly = gid >> logN;
    if (poly >= n_polys) return;
    const u64 q = primes[pm.prime_of[(first_poly + poly) % pm.period]].q;
    dst[gid] = mulhi64(splitmix64(seed ^ splitmix64(gid + (first_poly << logN))), q);
}
// key residues of fp64-engine primes are kept as doubles in HBM (exact: q < 2^47)
__global__ void k_key_to_engine(u64 *key, u64 n_polys, int logN, const PrimeDev *primes, int K)
{
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 poly = gid >> logN;
    if (poly >= n_polys) return;
    if (primes[poly % K].f64) {
        union { u64 u; double d; } c;
        c.d = u52_to_f64(key[gid]);
        key[gid] = c.u;
    }
}

// A finished key (k_key_to_engine's format) with the residues under the data primes multiplied by P^-1 (P = the special prime; the
// special prime's own residues are copied): what k_k3<TENSOR> multiplies the lifted digits by, so that its sums are sums * P^-1.
__global__ void k_key_scaled_copy(const u64 *key, u64 *out, u64 n_polys, int logN, const PrimeDev *primes, const FloorConst *fcs, int K)
{
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 poly = gid >> logN;
    if (poly >= n_polys) return;
    const int t = (int)(poly % K);
    u64 v = key[gid];
    if (t != K - 1) {
        const PrimeDev &P = primes[t];
        const FloorConst fc = fcs[(K - 1) * K + t];
        if (P.f64) {
            ArF64 ar;
            ar.q = (double)P.q; ar.qinv = 1.0 / (double)P.q;
            union { u64 u; double d; } c;
            c.u = v;
            c.d = ar.canon2(ar.mulmod_c(c.d, fc.inv_d, fc.inv_i));
            v = c.u;
        } else {
            ModU64 m; // (Barrett: this file is compiled once, whatever companion words the context's tables hold)
            m.q = P.q; m.cr0 = P.cr0; m.cr1 = P.cr1;
            v = mulmod(v, fc.inv, m);
        }
    }
    out[gid] = v;
}

// Companion words of the key residues under the u64-engine primes, appended to the key: [L_top][2][n_q][N] -- their Shoup quotients, or
// (fold: the context's u64-engine primes are 2^60 - c, modarith.h) the residues times 2^32
__global__ void k_key_quotients(const u64 *key, u64 *keyq, u64 n_dk, int logN, const PrimeDev *primes, int K, int n_q, PrimeMap qmap, int fold)
{
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 poly = gid >> logN; // (digit*2 + k) * n_q + slot
    if (poly >= n_dk * n_q) return;
    const int slot = (int)(poly % n_q), t = qmap.prime_of[slot];
    const u64 dk = poly / n_q;
    ArU64 ar;
    ar.q = primes[t].q; ar.two_q = 2 * ar.q; ar.cr0 = primes[t].cr0; ar.cr1 = primes[t].cr1; ar.ninv = ar.ninv_q = 0;
    const u64 kv = key[((dk * K + t) << logN) + (gid & (((u64)1 << logN) - 1))];
    keyq[gid] = fold ? barrett128((u128)kv << 32, ar.mod()) : ar.shoup_quotient(kv); // (exact quotient: k_k3's lazy runs rely on it)
}

} // namespace

// A count from the environment (HE355_CHUNK, HE355_LATENCY_MAX, HE355_LDS_MAX): false when the variable is unset, empty or not a decimal
// number -- the library's own rule then applies
static bool env_u64(const char *name, u64 &v)
{
    const char *s = std::getenv(name);
    if (!s || *s < '0' || *s > '9') return false;
    char *end = nullptr;
    errno = 0;
    const unsigned long long x = std::strtoull(s, &end, 10);
    if (*end || errno) return false;
    v = (u64)x;
    return true;
}

// 64 bits from the operating system's entropy source (the context's own encryptions of zero; the bridge's client seeds likewise)
static u64 os_seed()
{
    std::random_device rd;
    return ((u64)rd() << 32) ^ (u64)rd();
}

// In-run shader clock (bench.py's roofline.valu.sustained_mhz): ONE wave on a stream of its own reads the shader-cycle counter
// (s_memtime) and the constant 100 MHz counter (s_memrealtime), sleeps until `ticks_100mhz` of real time have passed -- a bound every
// path reaches, nothing else ends the loop -- and reads both again: clock = d(s_memtime) / d(s_memrealtime) x 100 MHz while the
// evaluator kernels of the probed region run beside it (/opt/skills/guides/MI355X_MICROARCH.md, "DVFS give-back" (6)).
__global__ void k_clock_probe(u64 ticks_100mhz, u64 *out)
{
    const u64 r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    u64 r = r0;
    while (r - r0 < ticks_100mhz) {
        __builtin_amdgcn_s_sleep(127);
        r = __builtin_amdgcn_s_memrealtime();
    }
    const u64 c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r - r0; }
}

class DeviceContext {
public:
    DeviceContext(const Params &p, int device) : P(p), device_(device)
    {
        // every per-prime table of the device side is sized kMaxPrimes (KernelEnv::prime_f64, PrimeMap, kernel argument lists)
        if (p.K + p.aux.size() + 1 > (size_t)kMaxPrimes) throw std::invalid_argument("too many primes for one device context (key chain + auxiliary primes exceed 64)");
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0) throw DeviceError("no HIP device available (the MI355X backend has no CPU fallback)");
        if (device < 0 || device >= count) throw DeviceError("invalid device ordinal");
        HIPCHECK(hipSetDevice(device));
        // a throw from here on (out of memory on a table) must give back the streams, events and tables made so far: the destructor of a
        // half-built object never runs, so the same teardown is called by hand
        try {
            init();
        } catch (...) {
            teardown();
            throw;
        }
    }
    ~DeviceContext() { teardown(); }

private:
    void init()
    {
        HIPCHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        HIPCHECK(hipStreamCreateWithFlags(&stream2_, hipStreamNonBlocking));
        HIPCHECK(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
        HIPCHECK(hipEventCreate(&ev0_));
        HIPCHECK(hipEventCreate(&ev1_));
        const size_t N = P.N, K = P.K;
        // BFV: the BEHZ auxiliary primes follow the key chain, then the plain modulus t (BatchEncoder's NTT mod t)
        const bool with_t = P.scheme == kSchemeBFV && P.plain_modulus > 2 && (P.plain_modulus - 1) % (2 * N) == 0;
        if (with_t) plain_tables_ = Params::make_prime_tables(P.plain_modulus, N, P.logn, true); // t < 2^32: the fp64 engine's
        t_index_ = with_t ? (int)(K + P.aux.size()) : -1;
        const size_t n_all = K + P.aux.size() + (with_t ? 1 : 0);
        std::vector<PrimeDev> pd(n_all);
        for (size_t i = 0; i < n_all; ++i) {
            const PrimeTables &pt = i < K ? P.primes[i] : i < K + P.aux.size() ? P.aux[i - K] : plain_tables_;
            Tw16 *dfwd = upload_owned(pt.fwd.data(), N), *dinv = upload_owned(pt.inv.data(), N);
            prime_dev_fill(pd[i], pt, N);
            pd[i].fwd = dfwd; pd[i].inv = dinv;
            env_.prime_f64[i] = pt.f64 ? 1 : 0;
            env_.prime_q[i] = pt.q;
        }
        k2_lift_masks(P, pd.data());
        d_primes_ = upload_owned(pd.data(), n_all);
        d_floor_ = upload_owned(floor_const_table(P).data(), K * K);
        env_.primes = d_primes_;
        env_.floor_consts = d_floor_;
        env_.N = (int)N; env_.logn1 = P.logn1; env_.K = (int)K; env_.Ltop = (int)P.Ltop; env_.scheme = P.scheme;
        env_.stream = stream_;
        env_.u64_fold = P.u64_fold;
        const char *ds = std::getenv("HE355_DUAL_STREAM");
        if (ds) dual_stream_ = ds[0] != '0';
        lim_.N = N; lim_.K = (int)K;
        u64 v = 0;
        if (env_u64("HE355_LATENCY_MAX", v)) set_latency_max(v);
        if (env_u64("HE355_LDS_MAX", v)) set_lds_max(v);
        if (env_u64("HE355_CHUNK", v) && v > 0) lim_.chunk = (size_t)v;
        int cus = 0;
        HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_));
        cus_ = cus > 0 ? (u64)cus : 1;
    }
    // drain, free the tables, the keys and the arenas, destroy the pool, then the events and streams (whatever of them exists)
    void teardown()
    {
        (void)hipSetDevice(device_);
        for (hipStream_t s : {stream_, stream2_, probe_stream_})
            if (s) (void)hipStreamSynchronize(s);
        for (void *p : owned_) pool_.raw_free(p);
        pool_.raw_free(d_relin_);
        pool_.raw_free(d_relin_scaled_);
        for (auto &kv : d_galois_) pool_.raw_free(kv.second);
        for (auto &kv : d_hoist_) pool_.raw_free(kv.second.p);
        for (Arena &a : arena_) pool_.raw_free(a.p);
        pool_.destroy();
        for (hipEvent_t e : {ev_fork_, ev_join_, ev0_, ev1_})
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {stream2_, probe_stream_, stream_})
            if (s) (void)hipStreamDestroy(s);
    }

public:
    void use() { HIPCHECK(hipSetDevice(device_)); }
    // ---- device memory (device_pool.h): slabs handed to callers come from the pool, the context's own tables / keys / arenas
    // are raw allocations; both are counted
    template <class T> void dmalloc(T *&p, size_t bytes) { p = static_cast<T *>(pool_.raw_malloc(bytes)); }
    // a device table the context owns until it goes (owned_): `count` elements, copied from `h` (null: left as allocated)
    template <class T> T *upload_owned(const T *h, size_t count)
    {
        T *d = nullptr;
        dmalloc(d, count * sizeof(T));
        owned_.push_back(d);
        if (h) HIPCHECK(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    void *pool_alloc(size_t bytes)
    {
        use();
        return pool_.alloc(bytes);
    }
    void pool_free(void *p)
    {
        switch (pool_.release(p)) {
        case DevicePool::kReleased: return;
        case DevicePool::kCached: throw std::invalid_argument("he355_free: this block was freed already");
        default: throw std::invalid_argument("he355_free: not a block this context allocated (he355_malloc of another context?)");
        }
    }
    // a pool block that goes back at the end of the caller's scope (device_pool.h)
    PoolBlock scoped_block(size_t bytes)
    {
        use();
        return PoolBlock(pool_, bytes);
    }
    DevicePool::Stats alloc_stats() const { return pool_.stats(); }
    // the counter blocks of every *_stats call, counted on the host where the calls branch and read by no launch
    struct Counters {
        he355_path_stats_t paths{};
        he355_hoist_stats_t hoist{};
        he355_poly_stats_t poly{};
        he355_raise_stats_t raise{};
        he355_cheb_stats_t cheb{};
        he355_bfv_route_stats_t routes{};
        he355_bfv_multiply_stats_t mul_routes{};
    };
    // the one read of a counter block (every *_stats call): its value, and the block back at zero where the caller asks
    template <class S> static S take_stats(S &counters, bool reset)
    {
        const S s = counters;
        if (reset) counters = S{};
        return s;
    }
    // which shape / schedule the key switches of this context took (he355_path_stats): counted per kernel sequence (one chunk of a batch)
    he355_path_stats_t path_stats(bool reset) { return take_stats(count_.paths, reset); }
    // which route the BFV PIR calls of this context took (he355_bfv_route_stats): counted on the host where the calls branch, read by no launch
    he355_bfv_route_stats_t bfv_route_stats(bool reset) { return take_stats(count_.routes, reset); }
    he355_poly_stats_t poly_stats(bool reset) { return take_stats(count_.poly, reset); }
    he355_raise_stats_t raise_stats(bool reset) { return take_stats(count_.raise, reset); }
    he355_cheb_stats_t cheb_stats(bool reset) { return take_stats(count_.cheb, reset); }
    size_t pool_trim() { sync(); return pool_.trim(); }
    hipStream_t stream() const { return stream_; }
    int device() const { return device_; }
    const KernelEnv &env() const { return env_; }
    // ---- what the call families use (the *.inc files he355_api.hip includes last): read access for the sequences that live there
    const Params &params() const { return P; }
    const KsLimits &limits() const { return lim_; }
    size_t chunk_limit() const { return lim_.chunk; }
    u64 compute_units() const { return cus_; }
    const u64 *public_key() const { return d_pk_; }
    const u64 *secret_key() const { return d_sk_; }
    Counters &counters() { return count_; }
    // the kBfv arena holding `bytes` (he355_bfv_multiply_plain's prepared plaintexts), or null where it does not fit
    u64 *bfv_arena(size_t bytes) { return try_reserve(&arena_[kBfv], 1, bytes) ? arena_[kBfv].p : nullptr; }
    void set_chunk(size_t c) { lim_.chunk = c ? c : 1; }
    void set_latency_max(u64 n) { lim_.set_latency_max(n); } // ~0: back to lat_limit()'s rule
    void set_level_walk(bool on) { level_walk_ = on; }
    void set_lds_max(u64 n) { lim_.set_lds_max(n); }

    size_t key_elems() const { return P.Ltop * 2 * P.K * P.N; }
    size_t n_q_primes() const
    {
        size_t n = 0;
        for (size_t i = 0; i < P.K; ++i) n += env_.prime_f64[i] == 0;
        return n;
    }
    size_t key_alloc_elems() const { return key_elems() + P.Ltop * 2 * n_q_primes() * P.N; } // key + Shoup quotients (u64-engine primes)

    void key_from_host(u64 **slot, const u64 *h_key)
    {
        use();
        if (!*slot) dmalloc(*slot, key_alloc_elems() * 8);
        HIPCHECK(hipMemcpyAsync(*slot, h_key, key_elems() * 8, hipMemcpyHostToDevice, stream_));
        key_finish(*slot);
    }
    void key_synthetic(u64 **slot, u64 seed)
    {
        use();
        if (!*slot) dmalloc(*slot, key_alloc_elems() * 8);
        PrimeMap pm;
        pm.period = (u32)P.K;
        for (size_t i = 0; i < P.K; ++i) pm.prime_of[i] = (unsigned char)i;
        const u64 n_polys = P.Ltop * 2 * P.K, total = n_polys * P.N;
        hipLaunchKernelGGL(k_fill_uniform, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, *slot, n_polys, P.logn, d_primes_, pm, seed, (u64)0);
        key_finish(*slot);
    }
    // KeyGenerator on the device: the key for key_id 1 (relinearization) or 2 + galois_elt, from the secret key set with
    // he355_set_secret_key; same bits as the host client's make_relin_key / make_galois_key for the same seed
    void key_generate(u64 **slot, u64 seed, uint32_t galois_elt /* 0: relinearization key */)
    {
        use();
        require_keyswitch();
        if (!d_sk_) throw std::invalid_argument("secret key not set");
        if (!*slot) dmalloc(*slot, key_alloc_elems() * 8);
        const uint32_t *perm_tab = galois_elt ? perm(galois_elt) : nullptr;
        u64 *scr = client_scratch((P.Ltop * P.K + P.K) * P.N);
        launch_keygen_kswitch(env_, *slot, scr, scr + P.Ltop * P.K * P.N, d_sk_, perm_tab, seed, seed, galois_elt ? 2 + (u64)galois_elt : 1);
        key_finish(*slot);
    }
    void key_finish(u64 *d_key)
    {
        const u64 n_polys = P.Ltop * 2 * P.K, total = n_polys * P.N;
        if (d_key == d_relin_) d_relin_scaled_ok_ = false; // the scaled copy follows the key
        for (auto &kv : d_hoist_) // ... and so does the permuted copy of a Galois key (hoist_key): rebuilt on its next use
            if (galois_key(kv.first) == d_key) kv.second.ok = false;
        key_quotients(d_key);
        hipLaunchKernelGGL(k_key_to_engine, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, d_key, n_polys, P.logn, d_primes_, (int)P.K);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(stream_));
    }
    void key_quotients(u64 *d_key) // Shoup quotients of the residues under the u64-engine primes (integers in either key format)
    {
        const int n_q = (int)n_q_primes();
        if (n_q) { // before the fp64 conversion below rewrites the other residues; these stay integers
            PrimeMap qm;
            qm.period = (u32)n_q;
            int k = 0;
            for (size_t i = 0; i < P.K; ++i)
                if (!env_.prime_f64[i]) qm.prime_of[k++] = (unsigned char)i;
            const u64 n_dk = P.Ltop * 2, tq = n_dk * n_q * P.N;
            hipLaunchKernelGGL(k_key_quotients, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, stream_, d_key, d_key + key_elems(), n_dk, P.logn, d_primes_,
                               (int)P.K, n_q, qm, P.u64_fold ? 1 : 0);
        }
    }
    u64 **relin_slot() { return &d_relin_; }
    u64 **galois_slot(uint32_t elt) { return &d_galois_[elt]; }
    const u64 *relin_key() const { return d_relin_; }
    // the relinearization key with its data-prime residues times P^-1 (k_key_scaled_copy), built on first use after every change of the key
    const u64 *relin_scaled()
    {
        if (!d_relin_scaled_ok_) {
            if (!d_relin_scaled_) dmalloc(d_relin_scaled_, key_alloc_elems() * 8);
            const u64 n_polys = P.Ltop * 2 * P.K, total = n_polys * P.N;
            hipLaunchKernelGGL(k_key_scaled_copy, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, d_relin_, d_relin_scaled_, n_polys, P.logn, d_primes_,
                               d_floor_, (int)P.K);
            key_quotients(d_relin_scaled_);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(stream_));
            d_relin_scaled_ok_ = true;
        }
        return d_relin_scaled_;
    }
    const u64 *galois_key(uint32_t elt) const
    {
        auto it = d_galois_.find(elt);
        return it == d_galois_.end() ? nullptr : it->second;
    }
    // The Galois key of `elt` with every residue polynomial (and its Shoup-quotient block) permuted in NTT form by elt^-1: what a hoisted
    // rotation multiplies the UNPERMUTED digits by (sum_j sigma(d_j) k_j = sigma(sum_j d_j sigma^-1(k_j))).  Built on first use, kept per
    // element, rebuilt after the element's key is installed again (key_finish); a second allocation the size of the key.
    const u64 *hoist_key(uint32_t elt)
    {
        HoistKey &hk = d_hoist_[elt];
        if (!hk.ok) {
            const u64 m = 2 * (u64)P.N;
            u64 ginv = 1;
            for (u64 x = 1; x < m; x += 2)
                if (((x * elt) & (m - 1)) == 1) { ginv = x; break; }
            const uint32_t *table = perm((uint32_t)ginv);
            if (!hk.p) {
                dmalloc(hk.p, key_alloc_elems() * 8);
                count_.hoist.key_bytes += key_alloc_elems() * 8;
            }
            launch_key_permute(env_, galois_key(elt), hk.p, table, key_alloc_elems() / P.N);
            HIPCHECK(hipGetLastError());
            hk.ok = true;
            ++count_.hoist.keys_permuted;
        }
        return hk.p;
    }
    void hoist_release_keys()
    {
        use();
        HIPCHECK(hipStreamSynchronize(stream_));
        for (auto &kv : d_hoist_) pool_.raw_free(kv.second.p);
        d_hoist_.clear();
        count_.hoist.key_bytes = 0;
    }
    he355_hoist_stats_t hoist_stats(bool reset)
    {
        const he355_hoist_stats_t s = take_stats(count_.hoist, reset);
        count_.hoist.key_bytes = s.key_bytes; // (the bytes are a level, not a count)
        return s;
    }
    const uint32_t *perm(uint32_t elt)
    {
        auto it = d_perm_.find(elt);
        if (it != d_perm_.end()) return it->second;
        const std::vector<uint32_t> h = P.galois_perm_ntt(elt);
        const uint32_t *d = d_perm_[elt] = upload_owned(h.data(), P.N);
        std::array<unsigned char, 32> rows{};
        for (size_t a = 0; a < ((size_t)1 << P.logn1) && a < rows.size(); ++a) rows[a] = (unsigned char)(h[a << kRowLog] >> kRowLog);
        perm_rows_[elt] = rows; // the one source row of every row of the permuted polynomial (the ring-in-LDS kernels take it with their arguments)
        return d;
    }

    const uint32_t *gather(uint32_t elt)
    {
        auto it = d_gather_.find(elt);
        if (it != d_gather_.end()) return it->second;
        const std::vector<uint32_t> h = P.galois_gather_coeff(elt);
        return d_gather_[elt] = upload_owned(h.data(), P.N);
    }

    void set_dual_stream(bool on) { dual_stream_ = on; }
    void fill_uniform(u64 *dst, u64 n_polys, const uint8_t *prime_of, u32 period, u64 seed, u64 first_poly = 0)
    {
        use();
        if (period == 0 || period > 64) throw std::invalid_argument("prime map period must be in [1, 64]");
        PrimeMap pm;
        pm.period = period;
        for (u32 i = 0; i < period; ++i) {
            if (prime_of[i] >= P.K) throw std::invalid_argument("prime index out of range");
            pm.prime_of[i] = prime_of[i];
        }
        const u64 total = n_polys * P.N;
        hipLaunchKernelGGL(k_fill_uniform, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, dst, n_polys, P.logn, d_primes_, pm, seed, first_poly);
        HIPCHECK(hipGetLastError());
    }

    // ---- per-op sequences ------------------------------------------------------------------------------
    void check_level(int L) const
    {
        if (L < 1 || (size_t)L > P.Ltop) throw std::invalid_argument("level out of range");
    }
    // plain [n][N] mod t -> dst [n][L][N]: the centred lift under primes 0 .. L-1 and its forward transform (he355_bfv_plain_to_ntt's definition)
    void plain_to_ntt(int L, u64 n, const u64 *src, u64 *dst)
    {
        launch_bfv_lift_plain(env_, L, n, src, dst, P.plain_modulus);
        launch_ntt_forward(env_, poly_view(dst, L, P.N, L), (u32)n);
    }
    // the forward transform of `items` items of `v`: the row pass alone where a fused kernel has run the column pass (cols), else all of it
    void forward_rows_or_full(bool cols, const PolyView &v, u32 items)
    {
        if (cols) launch_rows_fwd(env_, v, items);
        else launch_ntt_forward(env_, v, items);
    }
    void addsub(int L, int size, u64 n, const u64 *a, const u64 *b, Indexer ix, u64 *out, bool sub)
    {
        use();
        check_level(L);
        launch_addsub(env_, L, size, n, a, b, ix, out, sub);
        HIPCHECK(hipGetLastError());
    }
    void multiply(int L, u64 n, const u64 *a, const u64 *b, Indexer ix, u64 *out)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_multiply implements the CKKS (NTT-form) product");
        launch_mul3(env_, L, n, a, b, ix, out);
        HIPCHECK(hipGetLastError());
    }

    struct Scratch {
        KsBuffers ks;
        u64 *rlr; // [C][3][N]  tail of the rescale prime after the inverse row pass
        u64 *f;   // [C][3][L][N]
    };
    // ---- the context's grow-on-demand device buffers (Arena, device_pool.h), one per use: which buffer serves which call is fixed
    enum { kScratch0, kScratch1, // key-switch scratch, one per stream (scratch())
           kLat0, kLat1,         // partial sums of the digit-split K3 (latency shape), one per stream: chunks of the two are in flight together
           kRotTmp,              // intermediate ciphertexts of rotation chains (rotate, rotate_sum_by_node, rotate_each)
           kBfv,                 // the BFV multiply's operands and products; he355_bfv_multiply_plain's prepared plaintexts
           kClient,              // encrypt / decrypt / encode / decode / noise budget / key generation
           kGroups,              // the ring of group tables of the grouped key switches (upload_groups)
           kArenas };
    // at least `bytes` afterwards; contents are not kept.  Both streams are drained before the old block goes (no steady-state call grows
    // one: test_steady_state_operate_does_not_allocate).
    u64 *reserve(Arena &a, size_t bytes)
    {
        if (bytes <= a.bytes) return a.p;
        HIPCHECK(hipStreamSynchronize(stream_));
        HIPCHECK(hipStreamSynchronize(stream2_));
        pool_.raw_free(a.p);
        a = Arena{};
        dmalloc(a.p, bytes);
        a.bytes = bytes;
        return a.p;
    }
    // The one fit rule: the `count` arenas from `first` on hold `need` bytes each afterwards, or false -- not enough device memory.  What has
    // to grow is checked against 0.9 of the memory that is free now plus what this context can give back (the arenas being replaced, the
    // pool's cached blocks); a hipMalloc that fails all the same (another context or process took the memory between the query and the
    // call) is a "no" as well, not an error -- unless the caller has nothing smaller left to ask for (last_resort: the allocator's own error goes up).
    bool try_reserve(Arena *first, int count, size_t need, bool last_resort = false)
    {
        size_t grow = 0, reclaim = pool_.cached_bytes();
        for (Arena *a = first; a != first + count; ++a)
            if (need > a->bytes) { grow += need; reclaim += a->bytes; }
        size_t free_b = 0, total_b = 0;
        if (grow && hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)grow > 0.9 * (double)(free_b + reclaim)) return false;
        try {
            for (Arena *a = first; a != first + count; ++a) reserve(*a, need);
            return true;
        } catch (const OutOfDeviceMemory &) {
            if (last_resort) throw;
            return false;
        }
    }
    // Ciphertexts per chunk for a batch of n at level L: lim_.chunk (default 1024, HE355_CHUNK / he355_set_chunk), halved until the scratch
    // arena(s) it needs -- two when the batch is cut and the chunks alternate between the streams -- are RESERVED (try_reserve: growing one
    // arena frees only that one).  On return scratch(c, L, which) does not allocate.
    size_t chunk_ops(u64 n, int L, bool may_dual)
    {
        const size_t per_op = scratch_words_per_op(P.N, L) * 8;
        const size_t c = halve_until_fit(std::min<u64>(lim_.chunk, n ? n : 1), [&](size_t k) { return try_reserve(&arena_[kScratch0], (may_dual && n > k) ? 2 : 1, per_op * k, k == 1); });
        if (!c) throw OutOfDeviceMemory("HIP error: out of device memory: the key-switch scratch of one ciphertext (" + std::to_string(per_op) + " bytes) does not fit");
        return c;
    }
    Scratch scratch(size_t c, int L, int which = 0)
    {
        const size_t N = P.N, LN = (size_t)L * N;
        const size_t per_op = scratch_words_per_op(N, L);
        Scratch s;
        u64 *p = reserve(arena_[kScratch0 + which], per_op * c * 8);
        s.ks.c01 = p; p += c * 2 * LN; s.ks.c01_item_stride = 2 * LN;
        s.ks.c2n = p; p += c * LN;
        s.ks.c2r = p; p += c * LN;
        s.ks.d = p; p += c * (size_t)(L + 1) * LN;
        s.ks.t = p; p += c * 2 * LN;
        s.ks.tp = p; p += c * 2 * N;
        s.ks.tpr = p; p += c * 2 * N;
        s.ks.e = p; p += c * 2 * LN;
        s.rlr = p; p += c * 3 * N;
        s.f = p;
        return s;
    }

    // The shape rules (ks_shape.h) for a kernel environment of this context -- a BFV context's batch_env(0, true) is on the CKKS pipeline
    bool fuse_pays(const KernelEnv &e, u64 nc, int L) const { return he355::fuse_pays(ks_dims(e), nc, L); }
    bool level_sum_pays(const KernelEnv &e, int L, u64 n) const { return he355::level_sum_pays(ks_dims(e), lim_, L, n); }
    bool latency_shape(const KernelEnv &e, u64 nc) const { return he355::latency_shape(ks_dims(e), lim_, nc); }
    bool lds_shape(const KernelEnv &e, int L, u64 nc) const { return he355::lds_shape(ks_dims(e), lim_, L, nc); }
    KsShape ks_shape(const KernelEnv &e, int L, u64 nc, KsKind kind, bool out_apart) const { return he355::ks_shape(ks_dims(e), lim_, L, nc, kind, out_apart); }
    // scratch of the shape: the arena behind c01 holds k_lds_digits' partial products, (2L + 4) L N words per ciphertext, for every L <= 6
    u64 *lds_part(const Scratch &S, int L) const
    {
        const size_t need = (size_t)ks_lds_part_words(env_, L), have = scratch_words_per_op(P.N, L) - 2 * (size_t)L * P.N;
        if (need > have) throw std::logic_error("ring-in-LDS key switch: the arena is too small for the partial products");
        return S.ks.c2n;
    }

    struct KsSource {
        KsKind kind;
        const u64 *a = nullptr, *b = nullptr;
        Indexer ix{};
        const u64 *addend = nullptr; // Galois, optional [n][2][L][N]: may be `out` (the wave that reads a row of it writes that row, afterwards)
        uint32_t elt = 0;
        const uint32_t *table = nullptr;
        const u64 *key = nullptr;    // the relinearization key or the Galois key (grouped: the groups' keys)
        KsGroups groups{};
        bool coeff = false;          // a BFV context's coefficient-form ciphertexts (else the NTT-domain pipeline)
    };
    // the kernel environment of a batch on stream `which`
    // ntt: the NTT-domain (CKKS) pipeline whatever the context's scheme (a BFV context's tables are the same primes; only the data
    // representation differs)
    KernelEnv batch_env(int which = 0, bool ntt = false) const
    {
        KernelEnv env = env_;
        env.stream = which ? stream2_ : stream_;
        if (ntt) env.scheme = kSchemeCKKS;
        return env;
    }
    // The chunk loop of every batched op: `chunk` ciphertexts per step (chunk_ops(n, L, may_dual), or fewer), each with the scratch arena of
    // its stream.  With may_dual and a batch that is cut, the chunks alternate between the two streams, each with its own arena: the
    // ALU-bound key-product kernel of one chunk overlaps the HBM-bound multiply / digit-lift / floor kernels of the other.  The second
    // stream starts half a pipeline late: f(off, nc, which, scratch, fork) records `fork` (chunk 0 only, else null) once chunk 0's launches
    // are issued (the HBM shapes: after its K1 + K2) and stream2_ waits for it before its first chunk; from then on one stream's ALU-bound
    // kernels (K3, floor column pass) run beside the other's HBM-bound ones instead of beside their own kind (starting both streams
    // together measured slower: HISTORY.md).
    template <class F> void for_each_chunk(u64 n, int L, size_t chunk, bool may_dual, F &&f)
    {
        const bool dual = may_dual && n > chunk;
        u64 ci = 0;
        for (u64 off = 0; off < n; off += chunk, ++ci) {
            const int which = dual ? (int)(ci & 1) : 0;
            const bool fork = dual && ci == 0;
            f(off, std::min<u64>(chunk, n - off), which, scratch(std::min<u64>(chunk, n), L, which), fork ? ev_fork_ : nullptr);
            if (fork) HIPCHECK(hipStreamWaitEvent(stream2_, ev_fork_, 0));
        }
        if (dual) {
            HIPCHECK(hipEventRecord(ev_join_, stream2_));
            HIPCHECK(hipStreamWaitEvent(stream_, ev_join_, 0));
        }
    }
    // One key-switch batch: n ciphertexts described by `src` into `out` ([n][2][L][N]; rescale: [n][2][L-1][N]), chunk by chunk, each chunk
    // in the shape ks_shape picks and counted in he355_path_stats.  Returns true when a grouped source's level sum (KsGroups::sum_out) was
    // formed in k_k3; false where the chunks cannot hold whole groups on the fused path (the caller then sums the groups itself).
    bool key_switch_batch(int L, u64 n, const KsSource &src, bool rescale, u64 *out, bool may_dual)
    {
        const size_t N = P.N, LN = (size_t)L * N, out_per = 2 * (size_t)(rescale ? L - 1 : L) * N;
        const bool product = src.kind == KsKind::Product, grouped = src.kind == KsKind::Grouped;
        const bool galois = grouped || src.kind == KsKind::Galois;
        // A level sum is a read-modify-write of groups.sum_out WITHOUT atomics.  It is exact because (1) the launch shape gives one wave sole
        // ownership of a (ciphertext, polynomial, tile, row) of the sum across all groups of the launch (launch_k3 checks the whole-group
        // shape), and (2) every chunk of the level is queued on ONE stream, in order: grouped chunks never alternate over stream2_, and
        // grouped launches never take the four-wave or dual shapes.
        if (grouped && (rescale || may_dual || !k3_can_fuse(batch_env(0, true))))
            throw std::logic_error("grouped key switches: plain rotations on the fused pipeline, all chunks on one stream");
        // k_k3 (fused) and the ring-in-LDS kernels read the operand rows while they write results: only when `out` is a slab of its own
        bool out_apart = true;
        if (product && n) {
            u64 a_lo, a_n, b_lo, b_n;
            indexer_span(src.ix, n, a_lo, a_n, b_lo, b_n);
            out_apart = !ranges_overlap(out, n * out_per, src.a + a_lo * 2 * LN, (size_t)a_n * 2 * LN) && !ranges_overlap(out, n * out_per, src.b + b_lo * 2 * LN, (size_t)b_n * 2 * LN);
        } else if (src.kind == KsKind::Size3) {
            out_apart = !ranges_overlap(out, n * out_per, src.a, n * 3 * LN);
        }
        size_t chunk = chunk_ops(n, L, may_dual);
        KsGroups groups = src.groups;
        if (groups.sum_out) { // chunks of whole groups, each on the fused path (fuse_pays grows with the chunk), or no level sum in k_k3
            if (chunk < groups.group_size || !fuse_pays(batch_env(0, true), groups.group_size, L)) groups.sum_out = nullptr;
            else chunk -= chunk % groups.group_size;
        }
        for_each_chunk(n, L, chunk, may_dual, [&](u64 off, u64 nc, int which, Scratch S, hipEvent_t fork) {
            const KernelEnv env = batch_env(which, !src.coeff);
            KsBuffers &B = S.ks;
            if (!rescale) { B.c01 = out + off * 2 * LN; B.c01_item_stride = 2 * LN; }
            u64 *ro = rescale ? out + off * out_per : nullptr;
            const KsShape shape = ks_shape(env, L, nc, src.kind, out_apart);
            if (shape == KsShape::BfvCoeff) {
                const u64 *a = src.a + off * (galois ? 2 : 3) * LN;
                if (galois) {
                    launch_bfv_galois(env, L, nc, a, src.table, B.c01, B.c01_item_stride, B.c2n, src.addend ? src.addend + off * 2 * LN : nullptr);
                    bfv_key_switch(env, L, nc, S, B, src.key, B.c2n, LN);
                } else { // out = (c0, c1) of each size-3 ciphertext (read where they lie by the last kernel) + the key-switched c2
                    bfv_key_switch(env, L, nc, S, B, src.key, a + 2 * LN, 3 * LN, a, 3 * LN);
                }
            } else if (shape == KsShape::Lds) {
                // a ring that fits LDS: the tensor product / permutation, key switch and the add in two launches (the operands are read where they lie)
                ++count_.paths.ks_lds;
                LdsKsOperands o;
                if (product) {
                    o.mode = LDSKS_MUL; o.a = src.a; o.b = src.b; o.ix = src.ix; o.op_offset = off;
                } else if (galois) {
                    o.mode = LDSKS_GALOIS; o.a = src.a; o.op_offset = off; o.perm = src.table;
                    const std::array<unsigned char, 32> &rows = perm_rows_.at(src.elt);
                    std::copy(rows.begin(), rows.end(), o.perm_src_row);
                    o.add = src.addend ? src.addend + off * 2 * LN : nullptr; o.add_op_stride = 2 * LN;
                } else {
                    o.mode = LDSKS_PLAIN;
                    o.tgt = src.a + off * 3 * LN + 2 * LN; o.tgt_op_stride = 3 * LN;
                    o.add = src.a + off * 3 * LN; o.add_op_stride = 3 * LN;
                }
                launch_ks_lds(env, L, nc, o, src.key, lds_part(S, L), B.c01, B.c01_item_stride);
                if (rescale) launch_rescale_lds(env, L, 2, nc, B.c01, 2 * LN, ro);
            } else {
                const bool fused = shape == KsShape::Fused;
                if (groups.sum_out && !fused) throw std::logic_error("level sum: the fused key switch only");
                ++(fused ? count_.paths.ks_fused : shape == KsShape::Latency ? count_.paths.ks_latency : count_.paths.ks_unfused);
                if (fused && groups.sum_out) ++count_.paths.level_sum_launches_in_k3;
                // c0, c1 of the ciphertext the switched key part is added into: written by k_k1, or (in_k3) formed by k_k3 where it adds them
                // in -- k_k1 is HBM-bound and then reads and writes less, k_k3 is not and reads the operand rows instead of c01
                const bool in_k3 = fused && out_apart;
                K3Fuse ops{};
                if (in_k3 && product) {
                    ops.ta = src.a; ops.tb = src.b; ops.tix = src.ix; ops.t_op_offset = off;
                } else if (in_k3 && galois) {
                    // polynomial 1 is zero (4) or the addend's (5), and the epilogue gathers the permuted c0 from the input itself (grouped: the
                    // op's group names its source block; g_op_offset carries the chunk offset) -- k_k1 writes two rows instead of three
                    ops.c1_mode = src.addend ? 5 : 4;
                    ops.c1_src = src.addend ? src.addend + off * 2 * LN : nullptr;
                    ops.gsrc = src.a; ops.gperm = src.table; ops.gsrc_op_offset = grouped ? 0 : off;
                } else if (in_k3) { // c0, c1 and the NTT-form c2 read from the size-3 input where it lies (k_k1 only sends c2 through the inverse row pass)
                    ops.c1_mode = 3; ops.c1_src = src.a + off * 3 * LN;
                }
                K1Operands k1;
                k1.mode = product ? K1_MUL : galois ? K1_GALOIS : K1_CT3;
                k1.a = src.a; k1.b = src.b; k1.ix = src.ix; k1.op_offset = off; k1.perm = src.table; k1.addend = src.addend;
                k1.no_c01 = in_k3 && product; k1.no_c1 = in_k3 && !product; k1.no_c0n = in_k3 && galois;
                k1.groups = grouped ? &groups : nullptr;
                launch_k1(env, L, nc, k1, B);
                key_switch_tail(env, L, nc, S, shape, in_k3 && product ? relin_scaled() : src.key, ops, grouped ? &groups : nullptr, off, ro, fork);
                return;
            }
            if (fork) HIPCHECK(hipEventRecord(fork, env.stream));
        });
        HIPCHECK(hipGetLastError());
        return groups.sum_out != nullptr;
    }
    // An HBM-shape key switch after k_k1: K2, K3 and the mod-down into S.ks.c01, then (rescale_out) the rescale into rescale_out.
    // ops: K3Fuse's operand fields (k_k3 forms c0, c1); groups: per-group keys, op 0 of the chunk is op g_off of the grouped batch;
    // fork: recorded on the chunk's stream after K2
    void key_switch_tail(const KernelEnv &env, int L, u64 nc, const Scratch &S, KsShape shape, const u64 *key, const K3Fuse &ops,
                         const KsGroups *groups, u64 g_off, u64 *rescale_out, hipEvent_t fork)
    {
        const KsBuffers &B = S.ks;
        const size_t N = P.N, LN = (size_t)L * N;
        const int SP = (int)P.K - 1;
        const bool lat = shape == KsShape::Latency;
        launch_k2(env, L, nc, B, nullptr, 0, lat ? kLatTargets : 1);
        if (fork) HIPCHECK(hipEventRecord(fork, env.stream));
        if (lat) {
            // Few ciphertexts (HEBench's Latency category is batch 1: ckks eltwise .cpp:138-141): the throughput shape would leave one
            // wave walking all digits of a tile and one lane walking all targets of a column while the chip idles.  Same kernels,
            // unfused, with the serial loops dealt to more blocks: targets of a column over kLatTargets blocks (k_k2n, k_floor_colsn),
            // digits of a tile over kLatSplit (u64 engine: kLatSplitU64) single-wave blocks whose partial sums k_k3_combine adds (k_k3).
            u64 *part = reserve(arena_[kLat0 + (env.stream == stream2_ ? 1 : 0)], (size_t)std::max(kLatSplit, kLatSplitU64) * nc * 2 * (L + 1) * N * 8);
            launch_k3(env, L, nc, B, key, K3_ALL, nullptr, kLatSplit, part, kLatSplitU64);
            launch_k3_combine(env, L, nc, B, kLatSplit, part, kLatSplitU64);
        } else if (shape == KsShape::Unfused) {
            launch_k3(env, L, nc, B, key, K3_ALL, nullptr, 1, nullptr, 0, groups, g_off);
        } else {
            // fused: special prime first, its correction through the column pass, then the data primes with the mod-down finished
            // inside K3 (the sums never go to HBM)
            launch_k3(env, L, nc, B, key, K3_SPECIAL_ONLY, nullptr, 1, nullptr, 0, groups, g_off);
            K3Fuse f = ops;
            f.cols = B.e; f.c01 = B.c01; f.c01_item_stride = B.c01_item_stride; f.cols2 = nullptr; f.out = nullptr;
            if (rescale_out) {
                // Mod-down + rescale with ONE column pass and ONE row transform per target: only the prime the rescale divides out needs
                // the mod-down correction by itself (its tiles run first, mod-down only); for every other prime the two corrections are
                // combined in coefficient form, delta2 + P^-1 * delta1, inside one k_floor_colsn launch that reads both sources (the
                // special prime's sums and the divided-out prime's tail) -- 16 column passes per polynomial instead of 31, and the
                // mod-down correction slab is neither written for those primes nor read back.
                // A ct x ct multiply with operand-formed sums (ops.ta: the key residues carry P^-1, c0 and c1 are inside the sums) needs
                // no correction slab at all: the rescale wants the divided-out prime's mod-down result in coefficient form only, and
                // iNTT(sums') - P^-1 * delta1 is that residue, so its tiles go from the sums straight through the inverse row pass (raw_tail)
                // and the merged k_floor_colsn launch takes P^-1 * delta1 off once per column (sub2) -- 15 column passes, no
                // k_rows_inv_select, and the prime-(L-1) block of B.e is neither written nor read.
                const bool raw = ops.ta != nullptr;
                f.tt_lo = L - 1; f.tt_hi = L;
                if (raw) {
                    f.raw_tail = S.rlr;
                    launch_k3(env, L, nc, B, key, K3_DATA_ONLY, &f);
                    f.raw_tail = nullptr;
                } else {
                    launch_floor_cols(env, SP, 1, nc * 2, B.tpr, B.e, /*tgt_first*/ L - 1, /*dst_ntgt*/ L);
                    launch_k3(env, L, nc, B, key, K3_DATA_ONLY, &f);
                    launch_rows_inv_select(env, L - 1, nc * 2, B.c01 + (size_t)(L - 1) * N, (u64)LN, S.rlr);
                }
                launch_floor_cols(env, L - 1, L - 1, nc * 2, S.rlr, S.f, 0, L - 1, /*src2*/ B.tpr, SP, 1, /*sub2*/ raw);
                f.tt_lo = 0; f.tt_hi = L - 1; f.cols2 = S.f; f.out = rescale_out;
                launch_k3(env, L, nc, B, key, K3_DATA_ONLY, &f);
                return;
            }
            launch_floor_cols(env, SP, L, nc * 2, B.tpr, B.e);
            f.tt_lo = 0; f.tt_hi = L;
            launch_k3(env, L, nc, B, key, K3_DATA_ONLY, &f, 1, nullptr, 0, groups, g_off);
            return;
        }
        // the unfused mod-down: c01 += (t - NTT(e)) * P^-1, starting the rescale (tail of prime L-1) where one follows
        floor_step(env, SP, L, 2, nc, B.tpr, B.e, {B.t, 2 * LN, LN}, {B.c01, B.c01_item_stride, LN}, {B.c01, B.c01_item_stride, LN}, rescale_out ? L - 1 : -1, S.rlr,
                   lat ? kLatTargets : 1);
        if (rescale_out) rescale_tail(env, L, 2, nc, S, B.c01, 2 * LN, rescale_out);
    }
    void rescale_tail(const KernelEnv &env, int L, int size, u64 nc, const Scratch &S, const u64 *src, u64 src_op_stride, u64 *out)
    {
        const size_t N = P.N, LN = (size_t)L * N, L1N = (size_t)(L - 1) * N;
        floor_step(env, L - 1, L - 1, size, nc, S.rlr, S.f, {src, src_op_stride, LN}, {}, {out, (u64)size * L1N, L1N}, -1, nullptr, latency_shape(env, nc) ? kLatTargets : 1);
    }
    // One unfused floor step -- the key switch's mod-down (source: the special prime) or a rescale (source: the last data prime) -- as its
    // two launches: the column half, `src` [nc * n_src][N] (raw rows of the source prime) -> the corrections under n_tgt targets in `cols`
    // (tsplit > 1, the latency shape: a column's targets dealt to that many blocks), then the row half, out = (tsrc - NTT(cols)) * s^-1
    // (+ addend).  The three operands are strided (words from op to op and from polynomial to polynomial); tail_prime >= 0: the rows of that
    // prime also leave through the inverse row pass into `tail`, the source of the floor step that follows.
    template <class T> struct Strided {
        T *p = nullptr;
        u64 op_stride = 0, poly_stride = 0;
    };
    void floor_step(const KernelEnv &env, int src_prime, int n_tgt, int n_src, u64 nc, const u64 *src, u64 *cols, Strided<const u64> tsrc, Strided<const u64> addend,
                    Strided<u64> out, int tail_prime = -1, u64 *tail = nullptr, int tsplit = 1)
    {
        launch_floor_cols(env, src_prime, n_tgt, nc * (u64)n_src, src, cols, 0, 0, nullptr, 0, tsplit);
        FloorRowsArgs fr;
        fr.src_prime = src_prime; fr.n_tgt = n_tgt; fr.n_src = n_src;
        fr.cols = cols;
        fr.tsrc = tsrc.p; fr.tsrc_op_stride = tsrc.op_stride; fr.tsrc_poly_stride = tsrc.poly_stride;
        fr.addend = addend.p; fr.add_op_stride = addend.op_stride; fr.add_poly_stride = addend.poly_stride;
        fr.out = out.p; fr.out_op_stride = out.op_stride; fr.out_poly_stride = out.poly_stride;
        fr.tail_prime = tail_prime; fr.tail = tail;
        launch_floor_rows(env, nc, fr);
    }
    void require_keyswitch() const
    {
        if (P.K < 2) throw std::invalid_argument("encryption parameters do not support key switching");
    }

    void multiply_relin(int L, u64 n, const u64 *a, const u64 *b, Indexer ix, bool rescale, u64 *out)
    {
        use();
        check_level(L);
        require_keyswitch();
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_multiply_relin implements the CKKS pipeline");
        if (!d_relin_) throw std::invalid_argument("relinearization key not set");
        if (rescale && L < 2) throw std::invalid_argument("cannot rescale at the last level");
        KsSource src{KsKind::Product};
        src.a = a; src.b = b; src.ix = ix; src.key = d_relin_;
        key_switch_batch(L, n, src, rescale, out, dual_stream_);
    }
    void relinearize(int L, u64 n, const u64 *ct3, u64 *out, bool rescale = false)
    {
        use();
        check_level(L);
        require_keyswitch();
        if (!d_relin_) throw std::invalid_argument("relinearization key not set");
        const bool bfv = P.scheme == kSchemeBFV;
        if (bfv && rescale) throw std::invalid_argument("rescale is a CKKS operation");
        if (bfv && ranges_overlap(out, n * 2 * (size_t)L * P.N, ct3, n * 3 * (size_t)L * P.N)) throw std::invalid_argument("relinearize: `out` overlaps the size-3 input");
        if (rescale && L < 2) throw std::invalid_argument("cannot rescale at the last level");
        KsSource src{KsKind::Size3};
        src.a = ct3; src.key = d_relin_; src.coeff = bfv;
        key_switch_batch(L, n, src, rescale, out, false);
    }
    void plain_op(int L, int size, u64 n, const u64 *ct, const u64 *pt, Indexer ix, u64 *out, int mode)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("plaintext operands are NTT-form CKKS plaintexts");
        check_size(size, 1, 3);
        launch_plain_op(env_, L, size, n, ct, pt, ix, out, mode);
        HIPCHECK(hipGetLastError());
    }
    void mod_switch_drop(int L, int L_to, u64 n_polys, const u64 *in, u64 *out)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_mod_switch_drop is the CKKS modulus switch");
        if (L_to < 1 || L_to > L) throw std::invalid_argument("target level out of range");
        launch_drop_residues(env_, L, L_to, n_polys, in, out);
        HIPCHECK(hipGetLastError());
    }
    void sum(int L, int size, u64 n, const u64 *in, u64 *out)
    {
        use();
        check_level(L);
        check_size(size, 1, 3);
        if (n < 1) throw std::invalid_argument("nothing to sum");
        launch_sum_cts(env_, L, size, n, in, out);
        HIPCHECK(hipGetLastError());
    }
    void multiply_accumulate(int L, u64 rows, u64 cols, u64 inner, const u64 *a, u64 a_stride_i, u64 a_stride_k, const u64 *b, u64 b_stride_k,
                             u64 b_stride_j, u64 *out)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_multiply_accumulate implements the CKKS (NTT-form) product");
        if (inner < 1 || inner > 0x7fffffff) throw std::invalid_argument("inner dimension out of range");
        if (rows * cols == 0) return;
        launch_mul3_acc(env_, L, rows, cols, (int)inner, a, a_stride_i, a_stride_k, b, b_stride_k, b_stride_j, out);
        HIPCHECK(hipGetLastError());
    }
    void rescale(int L, int size, u64 n, const u64 *in, u64 *out)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_rescale is a CKKS operation");
        if (L < 2) throw std::invalid_argument("cannot rescale at the last level");
        check_size(size, 1, 3);
        const size_t N = P.N, LN = (size_t)L * N, L1N = (size_t)(L - 1) * N;
        const bool apart = !ranges_overlap(in, n * size * LN, out, n * size * L1N); // (the two-launch form's blocks of an op read all of its input)
        for_each_chunk(n, L, chunk_ops(n, L, false), false, [&](u64 off, u64 nc, int which, const Scratch &S, hipEvent_t) {
            const KernelEnv env = batch_env(which);
            const u64 *src = in + off * size * LN;
            u64 *dst = out + off * size * L1N;
            if (apart && lds_shape(env, L, nc)) {
                launch_rescale_lds(env, L, size, nc, src, (u64)size * LN, dst);
                return;
            }
            launch_rows_inv_select(env, L - 1, nc * size, src + (size_t)(L - 1) * N, LN, S.rlr);
            rescale_tail(env, L, size, nc, S, src, (u64)size * LN, dst);
        });
        HIPCHECK(hipGetLastError());
    }
    // `addend` (optional, [n][2][L][N]; may alias `out`): out = addend + galois(in) -- the add_inplace that follows
    // a rotation in accumulateCKKS/BFV and in the row-major MatMult is folded into the first kernel of the rotation.  No kernel writes
    // the addend unless it is `out`, so it may also be `in` itself (out = in + galois(in): bfv_expand's even children).
    // ntt_form (BFV contexts): the ciphertexts are held in NTT form (a rotation chain that was transformed on the way in runs on the fused
    // NTT-domain pipeline: accumulate, rotate_sum)
    void apply_galois(int L, u64 n, const u64 *in, uint32_t elt, u64 *out, const u64 *addend = nullptr, bool ntt_form = false)
    {
        use();
        check_level(L);
        require_keyswitch();
        if (!(elt & 1) || elt >= 2 * P.N) throw std::invalid_argument("Galois element is not valid");
        const u64 *key = galois_key(elt);
        if (!key) throw std::invalid_argument("Galois key not present");
        // every kernel of the pipeline reads `in` while later ones already write `out`: any overlap (not just in == out) corrupts the input
        if (ranges_overlap(in, n * 2 * (size_t)L * P.N, out, n * 2 * (size_t)L * P.N)) throw std::invalid_argument("apply_galois cannot run in place: `out` overlaps `in`");
        KsSource src{KsKind::Galois};
        src.a = in; src.addend = addend; src.elt = elt; src.key = key;
        src.coeff = P.scheme == kSchemeBFV && !ntt_form;
        src.table = src.coeff ? gather(elt) : perm(elt);
        key_switch_batch(L, n, src, false, out, false);
    }
    // the rotation plans of rotation_plan.h over the Galois keys this context holds: every refusal over a step and its keys is made there
    std::vector<int> rotation_terms(int step) const
    {
        return he355::rotation_terms(P, step, [this](uint32_t e) { return galois_key(e) != nullptr; });
    }
    RotTrie rotation_trie(const int *steps, u64 n_steps) const
    {
        return he355::rotation_trie(P, steps, n_steps, [this](uint32_t e) { return galois_key(e) != nullptr; });
    }
    // Evaluator::rotate_internal: the key of the step if present, otherwise its NAF terms one after the other (rotation_terms)
    void rotate(int L, u64 n, const u64 *in, int step, u64 *out, const u64 *addend = nullptr, bool ntt_form = false)
    {
        use();
        const size_t bytes = n * 2 * (size_t)L * P.N * 8;
        const std::vector<int> terms = rotation_terms(step); // (a missing key of ANY term is refused here: nothing is launched or reserved yet)
        const size_t m = terms.size();
        if (!m) { // no rotation: out = in (+ addend)
            if (addend) {
                Indexer ixp{};
                ixp.pairwise = 1;
                addsub(L, 2, n, in, addend, ixp, out, false);
            } else if (in != out) HIPCHECK(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, stream_));
            return;
        }
        if (terms[0] != step) { // NAF terms (a step with a key of its own is apply_galois itself, refusals included)
            if (ranges_overlap(in, bytes / 8, out, bytes / 8)) throw std::invalid_argument("rotate cannot run in place: `out` overlaps `in`");
            if (addend == out && m > 1) throw std::invalid_argument("rotate_add through several Galois steps cannot add in place");
        }
        u64 *rot_tmp = m > 1 ? reserve(arena_[kRotTmp], bytes) : nullptr;
        // ping-pong between out and the temporary so that the last rotation lands in out
        const u64 *cur = in;
        for (size_t t = 0; t < m; ++t) {
            u64 *dst = ((m - 1 - t) % 2 == 0) ? out : rot_tmp;
            apply_galois(L, n, cur, P.galois_elt_from_step(terms[t]), dst, t + 1 == m ? addend : nullptr, ntt_form); // the addend joins the last step only
            cur = dst;
        }
    }
    // The next region of `bytes` (a multiple of 256) of the context's table ring in HBM, for a small table a call uploads from the host with
    // a synchronous copy: every upload takes the next region, so a region is never rewritten while kernels that were launched with it may
    // still be running; when the ring wraps (or has to grow) the stream is drained first.  The copy is complete on return, whatever the
    // runtime does with pageable memory, and everything that reads the region is launched afterwards.
    unsigned char *table_ring(size_t bytes)
    {
        Arena &ring = arena_[kGroups];
        if (bytes > ring.bytes || groups_next_ + bytes > ring.bytes) {
            HIPCHECK(hipStreamSynchronize(stream_));
            if (bytes > ring.bytes / 4) reserve(ring, std::max<size_t>(bytes * 8, (size_t)64 << 10)); // (eight uploads' worth: always more than it held; reserve drains both streams)
            groups_next_ = 0;
        }
        unsigned char *d_tab = reinterpret_cast<unsigned char *>(ring.p) + groups_next_;
        groups_next_ += bytes;
        return d_tab;
    }
    // device copy of a level's group tables: [perm pointers | key pointers | src_block | mult], grown as needed
    struct GroupTables { KsGroups g; const u32 *d_mult; };
    GroupTables upload_groups(const std::vector<const uint32_t *> &perms, const std::vector<const u64 *> &keys, const std::vector<u32> &src_block,
                              const std::vector<u32> &mult, u32 group_size)
    {
        const size_t G = perms.size(), bytes = (G * (8 + 8 + 4 + 4) + 255) & ~(size_t)255;
        unsigned char *d_tab = table_ring(bytes);
        std::vector<unsigned char> h(bytes, 0);
        std::memcpy(h.data(), perms.data(), G * 8);
        std::memcpy(h.data() + G * 8, keys.data(), G * 8);
        std::memcpy(h.data() + G * 16, src_block.data(), G * 4);
        std::memcpy(h.data() + G * 20, mult.data(), G * 4);
        HIPCHECK(hipMemcpy(d_tab, h.data(), bytes, hipMemcpyHostToDevice));
        GroupTables t;
        t.g.perm = reinterpret_cast<const uint32_t *const *>(d_tab);
        t.g.key = reinterpret_cast<const u64 *const *>(d_tab + G * 8);
        t.g.src_block = reinterpret_cast<const u32 *>(d_tab + G * 16);
        t.g.group_size = group_size;
        t.d_mult = reinterpret_cast<const u32 *>(d_tab + G * 20);
        return t;
    }
    // NTT-form ciphertexts: out[g * gs + c] = apply_galois(in[src_block[g] * gs + c], element / key of group g), c < gs = groups.group_size,
    // g < n / gs groups.  groups.sum_out (level_sum_pays): k_k3 adds every group's ciphertext into the sum itself; chunks are then whole groups
    // (returns false where it could not: the scratch arenas hold less than one group per launch -- the caller then sums the groups itself)
    bool apply_galois_grouped(int L, u64 n, const u64 *in, const KsGroups &groups, u64 *out)
    {
        KsSource src{KsKind::Grouped};
        src.a = in; src.groups = groups;
        return key_switch_batch(L, n, src, false, out, false);
    }
    // out = in + sum_j rotate(in, steps[j]): the inner loop of the row-major MatMult (bfv row .cpp:519-531, ckks row .cpp:502-514:
    // result = base; result += rotate_rows(base, j * spacers) for j = 1 .. dim2-1).  Every rotation is what Evaluator::rotate_internal
    // computes -- the step's own Galois key if present, else its NAF terms applied least significant first -- and all of them start from
    // the same ciphertext, so two steps whose term sequences share a prefix share that prefix's intermediate CIPHERTEXT bit for bit
    // (same operations on the same input).  The term sequences form a trie; each node is key-switched once, from its parent's
    // ciphertext, and added to the running sum as often as steps end there (modular additions commute, so the order of the adds is
    // free).  For steps j * 2^k, j = 1 .. 2^m - 1, every prefix of a NAF sequence is the NAF sequence of a smaller j: 127 key
    // switches instead of 313 for the 128-column products of BASELINE configs[4].
    //
    // Round 4: the trie is walked LEVEL BY LEVEL, all nodes of a level in ONE kernel sequence (grouped key switches: every node's n
    // ciphertexts are a group with its own Galois element and key, KsGroups).  A node-by-node walk issues 127 sequences over 64
    // ciphertexts each at configs[4] -- the small-grid regime, 7.0-7.7 us per ciphertext and key switch; a level is 13-50 nodes, i.e.
    // 800-3200 ciphertexts per sequence: 4.8 us (tools/ks_probe.py, profiles/r04_bfv_gather_fold_negative.txt).  The walk runs in the
    // NTT domain on the fused CKKS pipeline for BOTH schemes: a BFV ciphertext is transformed once on the way in and the sum once on the
    // way out; in between every operation (Galois permutation, the key switch's digit lifts, key products and mod-down, modular
    // additions) is the same exact map on residues in either representation, since the NTT is a bijection that commutes with all of
    // them -- (t - delta) P^-1 in coefficient form and (NTT(t) - NTT(delta)) P^-1 in NTT form are the same polynomial.
    // Returns the number of key switches issued.  Not in place.
    u64 rotate_sum(int L, u64 n, const u64 *in, const int *steps, u64 n_steps, u64 *out)
    {
        use();
        check_level(L);
        const size_t per = 2 * (size_t)L * P.N, bytes = n * per * 8;
        if (ranges_overlap(in, n * per, out, n * per)) throw std::invalid_argument("rotate_sum cannot run in place: `out` overlaps `in`");
        const RotTrie tr = rotation_trie(steps, n_steps); // (every node's key is there: a missing one is refused before anything is allocated)
        const std::vector<RotNode> &trie = tr.nodes;
        if (!n) return 0;
        const KernelEnv nenv = batch_env(0, true);
        // node by node where that is the better shape: no fused path; CKKS batches so small that even the widest level stays within the
        // latency shape (digit-split k_k3: he355_set_latency_max) -- a BFV context has no latency shape, its levels always go grouped
        if (!level_walk_ || trie.size() == 1 || !k3_can_fuse(nenv) || latency_shape(env_, n * tr.widest) || n > 0xFFFFFFFFull / trie.size())
            return rotate_sum_by_node(L, n, in, tr, out);
        require_keyswitch();
        const bool bfv = P.scheme == kSchemeBFV;
        // the one block this walk holds at a time (the previous level's ciphertexts): back to the pool however the walk ends (stream-ordered
        // reuse: whatever takes the block next is queued behind these kernels)
        PoolBlock held;
        // level 0: the input in NTT form (BFV: a transformed copy), the running sum starts as (1 + steps of 0) x input
        const u64 *src = in;
        if (bfv) {
            held = PoolBlock(pool_, bytes);
            HIPCHECK(hipMemcpyAsync(held.get(), in, bytes, hipMemcpyDeviceToDevice, stream_));
            launch_ntt_forward(env_, poly_view(held.get(), 2 * L, P.N, L), (u32)n);
            src = held.get();
        }
        HIPCHECK(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, stream_));
        Indexer ixp{};
        ixp.pairwise = 1;
        for (u64 r = 0; r < trie[0].ends; ++r) addsub(L, 2, n, out, src, ixp, out, false);
        u64 switches = 0;
        for (size_t lv = 1; lv <= tr.depth(); ++lv) {
            const std::vector<int> &nodes = tr.levels[lv];
            const size_t G = nodes.size();
            std::vector<const uint32_t *> perms(G);
            std::vector<const u64 *> keys(G);
            std::vector<u32> src_block(G), mult(G);
            // The level's sum inside k_k3 (KsGroups::sum_out) where its grid shape fills the chip -- one block per (tile, eight ciphertexts),
            // each walking the level's groups -- and every chunk takes the fused path: the groups' ciphertexts that nothing starts from are
            // then never written, and k_sum_groups' pass over all of them (an HBM stream of its own, 6 % of configs[4]) is gone.
            const bool in_k3 = level_sum_pays(nenv, L, n) && n_steps < kGroupKeepBit;
            for (size_t g = 0; g < G; ++g) {
                const RotNode &nd = trie[(size_t)nodes[g]];
                perms[g] = perm(nd.elt);
                keys[g] = galois_key(nd.elt);
                src_block[g] = (u32)trie[(size_t)nd.parent].pos;
                mult[g] = (u32)nd.ends;
                if (in_k3 && !nd.kids.empty()) mult[g] |= kGroupKeepBit;
            }
            GroupTables gt = upload_groups(perms, keys, src_block, mult, (u32)n);
            PoolBlock cur(pool_, G * bytes); // (taken while the previous level's block is still held ...)
            if (in_k3) { gt.g.sum_out = out; gt.g.count = gt.d_mult; }
            if (apply_galois_grouped(L, G * n, src, gt.g, cur.get())) ++count_.paths.level_sums_in_k3;
            else { ++count_.paths.level_sums_by_kernel; launch_sum_groups(env_, L, n, (u32)G, cur.get(), gt.d_mult, out); }
            held = std::move(cur); // (... which leaves with `cur` at the end of this round, before the next level takes its own)
            src = held.get();
            switches += G;
        }
        held = PoolBlock();
        if (bfv) launch_ntt_inverse(env_, poly_view(out, 2 * L, P.N, L), (u32)n);
        HIPCHECK(hipGetLastError());
        return switches;
    }
    // the node-by-node walk (depth first, one key-switch sequence per node): the latency shape, the unfused sequence
    u64 rotate_sum_by_node(int L, u64 n, const u64 *in, const RotTrie &tr, u64 *out)
    {
        const std::vector<RotNode> &trie = tr.nodes;
        const size_t per = 2 * (size_t)L * P.N, bytes = n * per * 8;
        HIPCHECK(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, stream_));
        Indexer ixp{};
        ixp.pairwise = 1;
        for (u64 r = 0; r < trie[0].ends; ++r) addsub(L, 2, n, out, in, ixp, out, false); // steps of 0: the input once more
        if (trie.size() == 1) return 0;
        require_keyswitch();
        // one ciphertext slab per trie level (a node's ciphertext lives until its last child is done; a leaf needs one only when
        // several steps end there)
        u64 *rot_tmp = reserve(arena_[kRotTmp], tr.depth() * bytes);
        u64 switches = 0;
        // depth-first: (node, level of the node = number of terms applied)
        std::vector<std::pair<int, size_t>> stack;
        for (auto it = trie[0].kids.rbegin(); it != trie[0].kids.rend(); ++it) stack.push_back({*it, 1});
        while (!stack.empty()) {
            const auto [id, lvl] = stack.back();
            stack.pop_back();
            const RotNode &nd = trie[(size_t)id];
            const u64 *src = lvl == 1 ? in : rot_tmp + (lvl - 2) * n * per;
            const uint32_t e = nd.elt;
            if (nd.kids.empty() && nd.ends == 1) {
                apply_galois(L, n, src, e, out, out); // a leaf: the add_inplace rides the Galois step (sum += rotate(parent))
            } else {
                u64 *mine = rot_tmp + (lvl - 1) * n * per;
                apply_galois(L, n, src, e, mine);
                for (u64 r = 0; r < nd.ends; ++r) addsub(L, 2, n, out, mine, ixp, out, false);
                for (auto it = nd.kids.rbegin(); it != nd.kids.rend(); ++it) stack.push_back({*it, lvl + 1});
            }
            ++switches;
        }
        HIPCHECK(hipGetLastError());
        return switches;
    }
    // out[i] = rotate(in[i], steps[i]): the rotate_vector(dot_i, -i) loop of collapseCKKS (seal_context.cpp:389-392).  Every
    // ciphertext goes through its own NAF terms in its own order; ciphertexts whose t-th term is the same Galois element are
    // gathered and key-switched as one batch (a loop of single-ciphertext rotations is latency-bound: ~1 ms each at N=2^14).
    void rotate_each(int L, u64 n, const u64 *in, const int *steps, u64 *out)
    {
        use();
        check_level(L);
        if (!n) return;
        const size_t per = 2 * (size_t)L * P.N, bytes = n * per * 8;
        if (ranges_overlap(in, n * per, out, n * per)) throw std::invalid_argument("rotate_each cannot run in place: `out` overlaps `in`");
        std::vector<std::vector<int>> terms(n);
        size_t depth = 0;
        for (u64 i = 0; i < n; ++i) {
            terms[i] = rotation_terms(steps[i]);
            depth = std::max(depth, terms[i].size());
        }
        HIPCHECK(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, stream_));
        if (!depth) return;
        require_keyswitch();
        u64 *ga = reserve(arena_[kRotTmp], 2 * bytes), *gb = ga + n * per;
        for (size_t t = 0; t < depth; ++t) {
            std::map<uint32_t, std::vector<uint32_t>> groups; // Galois element -> ciphertexts whose t-th term it is
            u64 m_all = 0;
            for (u64 i = 0; i < n; ++i)
                if (t < terms[i].size()) { groups[P.galois_elt_from_step(terms[i][t])].push_back((uint32_t)i); ++m_all; }
            if (P.scheme == kSchemeCKKS && level_walk_ && k3_can_fuse(env_) && !latency_shape(env_, m_all) && groups.size() > 1) {
                // ONE grouped key-switch sequence for every ciphertext that has a t-th term (groups of one op, each with its own Galois
                // element and key, ordered by element so that neighbouring waves share key rows): the ciphertexts are read where they lie
                // in `out` (KsGroups::src_block), the results land compactly in gb and are scattered back.  A loop over the elements
                // issues one sequence per element over 1-14 ciphertexts each (logreg .cpp's collapse: 35 sequences for 100 samples).
                std::vector<const uint32_t *> perms;
                std::vector<const u64 *> keys;
                std::vector<u32> src_block, mult, order;
                for (const auto &g : groups)
                    for (uint32_t i : g.second) {
                        perms.push_back(perm(g.first));
                        keys.push_back(galois_key(g.first));
                        if (!keys.back()) throw std::invalid_argument("Galois key not present");
                        src_block.push_back(i);
                        mult.push_back(0);
                        order.push_back(i);
                    }
                const GroupTables gt = upload_groups(perms, keys, src_block, mult, 1);
                apply_galois_grouped(L, m_all, out, gt.g, gb);
                launch_move_cts(env_, out, gb, order.data(), m_all, per, true);
                continue;
            }
            for (const auto &g : groups) {
                const u64 m = g.second.size();
                launch_move_cts(env_, ga, out, g.second.data(), m, per, false);
                apply_galois(L, m, ga, g.first, gb);
                launch_move_cts(env_, out, gb, g.second.data(), m, per, true);
            }
        }
        HIPCHECK(hipGetLastError());
    }
    // The stream the context's own encryptions of zero draw from (accumulate with count 0): seeded from the OS at construction,
    // he355_set_zero_stream pins it (tests).
    void set_zero_stream(u64 seed, u64 first_index) { zero_seed_ = seed; zero_index_ = first_index; }
    // SEALContextWrapper::accumulateCKKS / accumulateBFV (seal_context.cpp:321-347, 289-319)
    void accumulate(int L, u64 n, u64 *inout, u64 count, u64 *tmp)
    {
        if (count == 0) {
            // the reference's else-branch (seal_context.cpp:312-316, 341-344): encryptor()->encrypt_zero(retval) -- a FRESH encryption
            // of zero at the first data level replaces every ciphertext.  SEAL returns it at the top level whatever the level of
            // the input was; a slab of lower-level ciphertexts cannot hold that, so only L == Ltop is accepted here.
            check_level(L);
            if ((size_t)L != P.Ltop) throw std::invalid_argument("accumulate with count 0 returns top-level encryptions of zero: the slab must be at the top level");
            encrypt(n, nullptr, zero_seed_, zero_index_, inout);
            zero_index_ += n;
            return;
        }
        // One ladder for both schemes: rotate by 1, 2, 4, .. and add, over the slots of a CKKS ciphertext (rotate_vector) or of one batching row
        // of a BFV one (rotate_rows); accumulateBFV (seal_context.cpp:289-319) then swaps the columns when the count reaches past a row.
        const bool bfv = P.scheme == kSchemeBFV;
        const u64 half = P.N / 2, row_count = std::min(count, half);
        const bool columns = bfv && count > half;
        int rot = 64 - __builtin_clzll(row_count);
        if (((u64)1 << (rot - 1)) == row_count) --rot;
        // BFV: the chain of rotate_rows + add_inplace (and the column swap) runs in the NTT domain on the fused pipeline the CKKS path uses
        // (Galois permutation in k_k1, mod-down inside k_k3, the latency shape for small batches): the ciphertexts are transformed
        // once on the way in and once on the way out, every step in between is the same exact map on residues in either
        // representation (see rotate_sum).  Two or more steps pay for the two transforms (20 transforms per key switch at L = 3).
        // Measured through the bridge (profiles/r04_bridge_phases.jsonl): it wins where the fused pipeline has a shape of its own -- the
        // latency shape (1 ciphertext at N = 2^14: 2.02 -> 1.59 ms) -- and in the throughput regime (1024 ciphertexts at N = 2^14:
        // 44.1 -> 38.9 ms); in between (64-80 ciphertexts at N <= 2^14) the BFV kernels' launches fill the chip better: 1.47 -> 1.77 ms.
        const KernelEnv nenv = batch_env(0, true);
        const bool ntt_chain = bfv && level_walk_ && rot + (columns ? 1 : 0) >= 2 && k3_can_fuse(nenv) && (latency_shape(nenv, n) || n * P.N >= ((u64)1 << 23));
        if (ntt_chain) launch_ntt_forward(env_, poly_view(inout, 2 * L, P.N, L), (u32)n);
        u64 *cur = inout, *nxt = tmp; // ping-pong: nxt = cur + rotate(cur), one pipeline per step and no separate add
        for (int i = 0; i < rot; ++i) {
            rotate(L, n, cur, 1 << i, nxt, cur, ntt_chain); // rotate_vector / rotate_rows + add_inplace
            std::swap(cur, nxt);
        }
        if (columns) {
            apply_galois(L, n, cur, (uint32_t)(2 * P.N - 1), nxt, cur, ntt_chain); // rotate_columns + add_inplace
            std::swap(cur, nxt);
        }
        if (cur != inout) HIPCHECK(hipMemcpyAsync(inout, cur, n * 2 * (size_t)L * P.N * 8, hipMemcpyDeviceToDevice, stream_));
        if (ntt_chain) launch_ntt_inverse(env_, poly_view(inout, 2 * L, P.N, L), (u32)n);
    }

    // ---- BFV ------------------------------------------------------------------------------------------
    // the per-level caches (behz_, crt_, bfv_delta_, bfv_noise_): the entry of level L, built on first use
    template <class T, class F> static const T &per_level(std::map<int, T> &cache, int L, F &&build)
    {
        auto it = cache.find(L);
        if (it == cache.end()) it = cache.emplace(L, build()).first;
        return it->second;
    }
    const BehzDev &behz(int L)
    {
        return per_level(behz_, L, [&] {
            const BehzHost H = P.behz_host(L); // the folded constants (he_params.cpp), as two flat arrays
            u64 *d = upload_owned(H.words.data(), H.words.size());
            double *ddev = upload_owned(H.doubles.data(), H.doubles.size());
            return H.view(d, ddev, P.K);
        });
    }
    // which route the BEHZ multiplies of this context took (he355_bfv_multiply_stats): counted below where bfv_multiply3 branches and from what
    // the launch_behz_* functions return, read by no launch; lds_limit is the device's answer, not a counter
    he355_bfv_multiply_stats_t bfv_multiply_stats(bool reset)
    {
        use();
        const auto lds_limit = behz_cols_lds_limit(env_);
        he355_bfv_multiply_stats_t s = take_stats(count_.mul_routes, reset);
        s.lds_limit = lds_limit;
        return s;
    }
    // out(i, j) = sum_k relinearize(multiply(a(i, k), b(k, j))): the multiply / relinearize_inplace / add_inplace loop of the BFV
    // CipherBatchAxis matrix product (bfv cipherbatchaxis .cpp:398-410) with the inner index as part of the batch -- one multiply and
    // one relinearization over rows * cols * k ciphertext pairs, then the sums over k (modular additions: any order, same residues).
    void bfv_multiply_relin_accumulate(int L, u64 rows, u64 cols, u64 inner, const u64 *a, u64 a_stride_i, u64 a_stride_k, const u64 *b,
                                       u64 b_stride_k, u64 b_stride_j, u64 *out)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeBFV) throw std::invalid_argument("he355_bfv_multiply_relin_accumulate needs a BFV context");
        if (inner < 1 || inner > 0x7fffffff) throw std::invalid_argument("inner dimension out of range");
        const u64 n = rows * cols;
        if (!n) return;
        const size_t LN = (size_t)L * P.N;
        // `out` is written after each pass over the inner index and the operands are read again by the next one
        const size_t a_cts = (size_t)((inner - 1) * a_stride_k + (rows - 1) * a_stride_i + 1), b_cts = (size_t)((inner - 1) * b_stride_k + (cols - 1) * b_stride_j + 1);
        if (ranges_overlap(out, n * 2 * LN, a, a_cts * 2 * LN) || ranges_overlap(out, n * 2 * LN, b, b_cts * 2 * LN))
            throw std::invalid_argument("he355_bfv_multiply_relin_accumulate: `out` overlaps an operand");
        const u64 kc = std::max<u64>(1, std::min<u64>(inner, (u64)4096 / n)); // inner indices per pass: about 4096 products in flight
        // (taken c3 then r2, as ever; a scope gives them back in reverse, r2 then c3 -- two size classes, so neither free list sees the order)
        const PoolBlock c3 = scoped_block(n * kc * 3 * LN * 8), r2 = scoped_block(n * kc * 2 * LN * 8);
        for (u64 k0 = 0; k0 < inner; k0 += kc) {
            const u64 kn = std::min<u64>(kc, inner - k0);
            Indexer3 ix{};
            ix.a_base = k0 * a_stride_k; ix.b_base = k0 * b_stride_k;
            ix.gs = n; ix.b1 = cols; ix.a_sg = a_stride_k; ix.a_si = a_stride_i; ix.b_sg = b_stride_k; ix.b_sj = b_stride_j;
            bfv_multiply3(L, n * kn, a, b, ix, c3.get());
            relinearize(L, n * kn, c3.get(), r2.get());
            launch_sum_cts(env_, L, 2, kn, r2.get(), out, n, k0 != 0);
        }
        HIPCHECK(hipGetLastError());
    }
    // Evaluator::bfv_multiply (BEHZ), size 2 x 2 -> 3, coefficient form
    void bfv_multiply(int L, u64 n, const u64 *a, const u64 *b, Indexer ix, u64 *out) { bfv_multiply3(L, n, a, b, to_ix3(ix), out); }
    // The two halves of the BEHZ multiply that its two paths share (vq / vb: the views of a polynomial set under q and under Bsk).
    // Extension to Bsk and the forward column passes of n_items operands (two polynomials each) into xq / xb: one kernel where the fused shape applies
    void behz_extend_fwd_cols(const BehzDev &Z, const BehzSrc &src, bool fuse_cols, u64 n_items, u64 *xq, u64 *xb, PolyView vq, PolyView vb)
    {
        if (fuse_cols) {
            ++count_.mul_routes.cols_fused;
            count_.mul_routes.cols_exact += launch_behz_extend_cols(env_, Z, src, n_items, xq, xb);
        } else {
            ++count_.mul_routes.cols_unfused;
            count_.mul_routes.coef_wide += launch_behz_extend(env_, Z, src, n_items, xq, xb);
            vq.base = xq; launch_cols_fwd(env_, vq, (u32)(n_items * 2));
            vb.base = xb; launch_cols_fwd(env_, vb, (u32)(n_items * 2));
        }
    }
    // the inverse column passes of nc products (three polynomials each) and steps (6)-(8) into `out`: again one kernel where it applies
    void behz_inv_cols_floor(const BehzDev &Z, bool fuse_cols, u64 nc, u64 *dq, u64 *ds, u64 *out, PolyView vq, PolyView vb)
    {
        if (fuse_cols) {
            ++count_.mul_routes.cols_fused;
            count_.mul_routes.cols_exact += launch_behz_cols_floor_sk(env_, Z, nc, dq, ds, out);
        } else {
            ++count_.mul_routes.cols_unfused;
            vq.base = dq; launch_cols_inv(env_, vq, (u32)(nc * 3));
            vb.base = ds; launch_cols_inv(env_, vb, (u32)(nc * 3));
            count_.mul_routes.coef_wide += launch_behz_floor_sk(env_, Z, nc, dq, ds, out);
        }
    }
    void bfv_multiply3(int L, u64 n, const u64 *a, const u64 *b, Indexer3 ix, u64 *out)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeBFV) throw std::invalid_argument("he355_bfv_multiply needs a BFV context");
        if (!n) return;
        const BehzDev &Z = behz(L);
        const size_t N = P.N, S = (size_t)Z.nB + 1;
        PolyView vq{}, vb{};
        for (int i = 0; i < L; ++i) vq.prime_of[i] = (unsigned char)i;
        for (size_t j = 0; j < S; ++j) vb.prime_of[j] = Z.bsk_prime[j];
        vq.polys_per_item = L; vq.item_stride = (u64)L * N;
        vb.polys_per_item = (int)S; vb.item_stride = (u64)S * N;
        const bool fuse_cols = behz_cols_fusable(env_, Z);
        BehzSrc src{};
        src.a = a; src.b = b; src.ix = ix;
        const BehzLists g = behz_lists(ix, n, L, S, N); // the distinct operands and the words either path takes (behz_lists.h)
        src.I = g.I; src.J = g.J; src.na = g.na;
        // a chunk's results are written before the next chunk's operands are read: `out` needs a slab of its own
        if (ranges_overlap(out, (size_t)n * 3 * L * N, a, g.a_cts * 2 * L * N) || ranges_overlap(out, (size_t)n * 3 * L * N, b, g.b_cts * 2 * L * N))
            throw std::invalid_argument("he355_bfv_multiply: `out` overlaps an operand");
        bool lists = g.may_list;
        Arena &arena = arena_[kBfv];
        size_t c = std::min<size_t>(lim_.chunk, (size_t)n);
        if (lists) {
            const size_t cl = halve_until_fit(c, [&](size_t k) { return try_reserve(&arena, 1, (g.e_words + g.per_res * k) * 8); });
            lists = cl != 0; // else: the operand set does not fit beside one result -- per-pair path below, from one result per chunk
            c = lists ? cl : 1;
        }
        if (lists) {
            src.lists = 1;
            ++count_.mul_routes.calls_lists;
            u64 *eq = arena.p, *eb = eq + (size_t)g.n_cts * 2 * L * N, *dq = eb + (size_t)g.n_cts * 2 * S * N, *ds = dq + c * 3 * L * N;
            behz_extend_fwd_cols(Z, src, fuse_cols, g.n_cts, eq, eb, vq, vb);
            vq.base = eq; launch_rows_fwd(env_, vq, (u32)(g.n_cts * 2));
            vb.base = eb; launch_rows_fwd(env_, vb, (u32)(g.n_cts * 2));
            for (u64 off = 0; off < n; off += c) {
                const u64 nc = std::min<u64>(c, n - off);
                ++count_.mul_routes.chunks;
                ++(launch_behz_tensor_inv(env_, Z, src, nc, off, eq, eb, dq, ds) ? count_.mul_routes.inv_dual : count_.mul_routes.inv_split);
                behz_inv_cols_floor(Z, fuse_cols, nc, dq, ds, out + off * 3 * (size_t)L * N, vq, vb);
            }
            HIPCHECK(hipGetLastError());
            return;
        }
        c = halve_until_fit(c, [&](size_t k) { return try_reserve(&arena, 1, g.per_op * k * 8); });
        if (!c) throw OutOfDeviceMemory("HIP error: out of device memory: the BFV multiply scratch of one ciphertext does not fit");
        ++count_.mul_routes.calls_pairs;
        u64 *xq = arena.p, *xb = xq + c * 4 * L * N, *dq = xb + c * 4 * S * N, *ds = dq + c * 3 * L * N;
        for (u64 off = 0; off < n; off += c) {
            const u64 nc = std::min<u64>(c, n - off);
            // extension to Bsk and forward column passes, then per (op, residue, row) ONE kernel for the forward row pass of the four
            // polynomials, the dyadic tensor and the inverse row pass of the three products (k_behz_rows_tensor), then the inverse column
            // passes and steps (6)-(8)
            src.op_offset = off;
            behz_extend_fwd_cols(Z, src, fuse_cols, nc * 2, xq, xb, vq, vb);
            ++count_.mul_routes.chunks;
            ++(launch_behz_rows_tensor(env_, Z, nc, xq, xb, dq, ds) ? count_.mul_routes.rows_dual : count_.mul_routes.rows_split);
            behz_inv_cols_floor(Z, fuse_cols, nc, dq, ds, out + off * 3 * (size_t)L * N, vq, vb);
        }
        HIPCHECK(hipGetLastError());
    }
    // key switching for BFV: the target is in coefficient form; result added into c01 (coefficient form)
    void bfv_key_switch(const KernelEnv &env, int L, u64 nc, const Scratch &S, const KsBuffers &B, const u64 *key, const u64 *target,
                        u64 target_op_stride, const u64 *add01 = nullptr, u64 add01_item_stride = 0)
    {
        launch_k2(env, L, nc, B, target, target_op_stride);
        launch_k3(env, L, nc, B, key);
        launch_bfv_tail_sp(env, nc * 2, B.tpr, S.rlr);
        launch_bfv_tail_fin(env, L, nc, B.t, S.rlr, B.c01, B.c01_item_stride, add01, add01_item_stride);
    }
    // ---- client side on the device -----------------------------------------------------
    void set_public_key(const u64 *h_pk) // [2][K][N], NTT form
    {
        use();
        const size_t bytes = 2 * P.K * P.N * 8;
        if (!d_pk_) d_pk_ = upload_owned(h_pk, 2 * P.K * P.N);
        else HIPCHECK(hipMemcpy(d_pk_, h_pk, bytes, hipMemcpyHostToDevice));
    }
    void set_secret_key(const u64 *h_sk) // [K][N], NTT form
    {
        use();
        const size_t bytes = P.K * P.N * 8;
        if (!d_sk_) d_sk_ = upload_owned(h_sk, P.K * P.N);
        else HIPCHECK(hipMemcpy(d_sk_, h_sk, bytes, hipMemcpyHostToDevice));
    }
    u64 *client_scratch(size_t elems) { return reserve(arena_[kClient], elems * 8); }
    static PolyView poly_view(u64 *base, int polys_per_item, size_t N, int period)
    {
        if (polys_per_item > 64) throw std::invalid_argument("too many polynomials per item");
        PolyView v;
        v.base = base; v.item_stride = (u64)polys_per_item * N; v.polys_per_item = polys_per_item; v.pad_ = 0;
        for (int i = 0; i < polys_per_item; ++i) v.prime_of[i] = (unsigned char)(i % period);
        return v;
    }
    // Encryptor::encrypt (asymmetric) of n plaintexts: CKKS plain [n][Ltop][N] NTT form, BFV plain [n][N] mod t;
    // out [n][2][Ltop][N].  Ciphertext r uses the counter-based streams of index first_index + r (client/sampler.h).
    // plain == nullptr: Encryptor::encrypt_zero (the plaintext term is skipped: adding the zero plaintext changes nothing).
    void encrypt(u64 n, const u64 *plain, u64 seed, u64 first_index, u64 *out)
    {
        use();
        if (!d_pk_) throw std::invalid_argument("public key not set");
        const size_t N = P.N, K = P.K, L = P.Ltop;
        const bool ckks = P.scheme == kSchemeCKKS;
        const u64 cmax = 32;
        // per ciphertext: u K, e 2K, z 2K (BFV), tail 2, cols 2L polys
        u64 *base = client_scratch(cmax * (K + 2 * K + 2 * K + 2 + 2 * L) * N);
        u64 *u = base, *e = u + cmax * K * N, *z = e + cmax * 2 * K * N, *tpr = z + cmax * 2 * K * N, *cols = tpr + cmax * 2 * N;
        for (u64 off = 0; off < n; off += cmax) {
            const u64 c = std::min<u64>(cmax, n - off);
            u64 *o = out + off * 2 * L * N;
            launch_enc_sample(env_, c, seed, first_index + off, u, e);
            launch_ntt_forward(env_, poly_view(u, (int)K, N, (int)K), (u32)c);
            if (ckks) {
                launch_ntt_forward(env_, poly_view(e, (int)(2 * K), N, (int)K), (u32)c);
                launch_enc_mul_pk(env_, c, u, d_pk_, e, true); // z := u*pk + NTT(e), in the e buffer
                if (K > 1) {
                    const int SP = (int)K - 1;
                    launch_rows_inv_select(env_, SP, c * 2, e + (size_t)SP * N, (u64)K * N, tpr);
                    floor_step(env_, SP, (int)L, 2, c, tpr, cols, {e, 2 * K * N, K * N}, {}, {o, 2 * L * N, L * N});
                } else {
                    HIPCHECK(hipMemcpyAsync(o, e, c * 2 * N * 8, hipMemcpyDeviceToDevice, stream_));
                }
                Indexer pw{};
                pw.b1 = 1; pw.pairwise = 1;
                if (plain) launch_plain_op(env_, (int)L, 2, c, o, plain + off * L * N, pw, o, 1); // c0 += plain
            } else {
                launch_enc_mul_pk(env_, c, u, d_pk_, z, false);
                launch_ntt_inverse(env_, poly_view(z, (int)(2 * K), N, (int)K), (u32)c);
                Indexer pw{};
                pw.b1 = 1; pw.pairwise = 1;
                launch_addsub(env_, (int)K, 2, c, z, e, pw, z, false);
                if (K > 1) launch_divround_last_coeff(env_, c * 2, z, o);
                else HIPCHECK(hipMemcpyAsync(o, z, c * 2 * N * 8, hipMemcpyDeviceToDevice, stream_));
                if (plain) launch_bfv_addsub_plain(env_, (int)L, 2, c, o, plain + off * N, pw, o, bfv_delta((int)L), false); // c0 += Delta(plain), in place
            }
        }
        HIPCHECK(hipGetLastError());
    }
    // ---- BFV level operations (he355_kernels_bfv_level.hip) ---------------------------------------------------------------
    // the constants of Delta_L, cached per level as crt_tables(L) caches its own (host side: they travel as a kernel argument)
    const BfvDeltaConst &bfv_delta(int L) { return per_level(bfv_delta_, L, [&] { return bfv_delta_const(env_.prime_q, L, P.plain_modulus); }); }
    // q_j^-1 mod q_i, floor(q_j / 2) mod q_i for i < j < Ltop: one device table for every (L, L_to), built on first use
    const BfvDropConst *bfv_drop_table_dev()
    {
        if (d_bfv_drop_) return d_bfv_drop_;
        const std::vector<BfvDropConst> tab = bfv_drop_table(env_.prime_q, (int)P.Ltop, P.u64_fold);
        return d_bfv_drop_ = upload_owned(tab.data(), tab.size());
    }
    // the ciphertexts / plaintexts a batch of n results reads: [lo, hi] of the indexer's operand 0 / operand 1
    static void indexer_span(const Indexer &ix, u64 n, u64 &a_lo, u64 &a_n, u64 &b_lo, u64 &b_n)
    {
        a_lo = idx_a(ix, 0); a_n = idx_a(ix, n - 1) - a_lo + 1;
        b_lo = ix.b_base; b_n = ix.pairwise ? n : std::min<u64>(n, ix.b1);
    }
    const CrtTablesDev &crt_tables(int L)
    {
        return per_level(crt_, L, [&] {
            const CrtTablesHost c = crt_tables_host(P, L); // one block (device_tables.h)
            const u64 *d = upload_owned(c.h.data(), c.h.size());
            CrtTablesDev t;
            t.L = L; t.words = c.words; t.Q = d; t.halfQ = d + c.o_half; t.punct = d + c.o_punct; t.inv = d + c.o_inv;
            t.Qd = c.Qd; t.t = P.plain_modulus;
            return t;
        });
    }
    // Decryptor::decrypt of n size-`size` ciphertexts at level L: CKKS -> [n][L][N] NTT-form plaintext (the phase);
    // BFV -> [n][N] coefficients mod t
    void decrypt(int L, int size, u64 n, const u64 *ct, u64 *out)
    {
        use();
        check_level(L);
        if (!d_sk_) throw std::invalid_argument("secret key not set");
        check_size(size, 2, 3);
        const size_t N = P.N;
        if (P.scheme == kSchemeCKKS) {
            launch_dot_sk(env_, L, size, n, ct, d_sk_, out);
            HIPCHECK(hipGetLastError());
            return;
        }
        if (L > 16) throw std::invalid_argument("BFV decryption supports up to 16 data primes");
        const CrtTablesDev &crt = crt_tables(L);
        const u64 cmax = 64;
        u64 *tmp = client_scratch(cmax * ((size_t)size * L + L) * N), *phase = tmp + cmax * (size_t)size * L * N;
        for (u64 off = 0; off < n; off += cmax) {
            const u64 c = std::min<u64>(cmax, n - off);
            HIPCHECK(hipMemcpyAsync(tmp, ct + off * size * L * N, c * size * L * N * 8, hipMemcpyDeviceToDevice, stream_));
            launch_ntt_forward(env_, poly_view(tmp, size * L, N, L), (u32)c);
            launch_dot_sk(env_, L, size, c, tmp, d_sk_, phase);
            launch_ntt_inverse(env_, poly_view(phase, L, N, L), (u32)c);
            launch_bfv_scale_round(env_, c, phase, out + off * N, crt);
        }
        HIPCHECK(hipGetLastError());
    }
    // Decryptor::invariant_noise_budget of n size-`size` BFV ciphertexts at level L: budget [n] int32, noise_bits [n] int32 or null.
    // Per chunk: polynomials 1 .. size-1 into scratch, forward transform, Horner with the NTT-form secret key (without the constant term),
    // inverse transform, then k_bfv_noise_bits adds c0 in coefficient form -- one forward transform and one slab copy less per ciphertext
    // than decrypt() spends on the same phase -- and gathers the per-ciphertext maximum in `budget`, which k_bfv_noise_finish turns into
    // the budget in place.  Everything on stream_, like decrypt().
    const BfvNoiseConst &bfv_noise(int L) { return per_level(bfv_noise_, L, [&] { return bfv_noise_const(env_.prime_q, L, P.plain_modulus); }); }
    // Ciphertexts per chunk: 2^21 coefficients' worth (64 at N = 32768, as decrypt(); 256 at N = 8192), at most 1024 -- 64 ciphertexts of a
    // small ring are one wave per SIMD for k_bfv_noise_bits, which then waits on its own dependent instructions (profiles/bfv_noise.txt) --
    // and never more than the batch chunk (he355_set_chunk), so a test can cut a small batch.
    u64 noise_chunk(u64 n) const
    {
        const u64 by_ring = std::min<u64>(1024, std::max<u64>(64, ((u64)1 << 21) / P.N));
        return std::max<u64>(1, std::min<u64>(n, std::min<u64>(by_ring, lim_.chunk)));
    }
    void bfv_noise_budget(int L, int size, u64 n, const u64 *ct, int32_t *budget, int32_t *noise_bits)
    {
        use();
        check_level(L);
        if (L > kBfvNoiseMaxL) throw std::invalid_argument("the BFV noise budget supports up to 16 data primes");
        check_size(size, 2, 3);
        if (!d_sk_) throw std::invalid_argument("secret key not set");
        if (!n) return;
        if (!ct || !budget) throw std::invalid_argument("he355_bfv_noise_budget: null ciphertexts or null budget output");
        const size_t N = P.N, LN = (size_t)L * N;
        const CrtTablesDev &crt = crt_tables(L);
        const BfvNoiseConst &nc = bfv_noise(L);
        const u64 cmax = noise_chunk(n);
        u64 *tmp = client_scratch(cmax * (size_t)size * LN), *part = tmp + cmax * (size_t)(size - 1) * LN;
        HIPCHECK(hipMemsetAsync(budget, 0, n * sizeof(int32_t), stream_));
        for (u64 off = 0; off < n; off += cmax) {
            const u64 c = std::min<u64>(cmax, n - off);
            const u64 *src = ct + off * size * LN;
            launch_bfv_noise_take(env_, L, size, c, src, tmp);
            launch_ntt_forward(env_, poly_view(tmp, (size - 1) * L, N, L), (u32)c);
            launch_bfv_noise_dot_sk(env_, L, size, c, tmp, d_sk_, part);
            launch_ntt_inverse(env_, poly_view(part, L, N, L), (u32)c);
            launch_bfv_noise_bits(env_, size, c, part, src, budget + off, crt, nc);
        }
        launch_bfv_noise_finish(env_, n, budget, noise_bits, nc.q_bits);
        HIPCHECK(hipGetLastError());
    }
    // the `b` halves [L_top][K][N] of the Galois key of `galois_elt`, its `a` halves drawn from the public a_seed: the whole key is made in a
    // pool block by the key generator's own launches, the halves copied out.  Installs nothing.
    void keygen_galois_seeded(uint32_t galois_elt, u64 a_seed, u64 noise_seed, u64 *d_b)
    {
        use();
        if (!d_sk_) throw std::invalid_argument("he355_keygen_galois_seeded: secret key not set (he355_set_secret_key)");
        if (!d_b) throw std::invalid_argument("he355_keygen_galois_seeded: null output");
        const size_t KN = P.K * P.N;
        const PoolBlock key = scoped_block(P.Ltop * 2 * KN * 8);
        const uint32_t *perm_tab = perm(galois_elt);
        u64 *scr = client_scratch((P.Ltop * P.K + P.K) * P.N);
        launch_keygen_kswitch(env_, key.get(), scr, scr + P.Ltop * KN, d_sk_, perm_tab, a_seed, noise_seed, 2 + (u64)galois_elt);
        for (size_t j = 0; j < P.Ltop; ++j) HIPCHECK(hipMemcpyAsync(d_b + j * KN, key.get() + j * 2 * KN, KN * 8, hipMemcpyDeviceToDevice, stream_));
        HIPCHECK(hipGetLastError());
    }
    // he355_set_galois_key of the key whose `b` halves are h_b and whose `a` halves are a_seed's: uploaded, generated, finished
    void key_from_seeded(uint32_t galois_elt, const u64 *h_b, u64 a_seed)
    {
        use();
        u64 **slot = galois_slot(galois_elt);
        if (!*slot) dmalloc(*slot, key_alloc_elems() * 8);
        const size_t KN = P.K * P.N;
        for (size_t j = 0; j < P.Ltop; ++j) HIPCHECK(hipMemcpyAsync(*slot + j * 2 * KN, h_b + j * KN, KN * 8, hipMemcpyHostToDevice, stream_));
        launch_bfv_seeded_gen(env_, (int)P.K, P.Ltop, a_seed, client::keygen_stream(2 + (u64)galois_elt, 0, P.K, 0), P.K + 1, *slot + KN, 2 * KN, nullptr);
        key_finish(*slot);
    }
    // ---- encoders (CKKSEncoder / BatchEncoder) -------------------------------------------------------------------
    const EncTablesDev &enc_tables()
    {
        if (enc_.slot_index) return enc_;
        std::vector<uint32_t> si;
        client::build_slot_index(P.N, si);
        enc_.slot_index = upload_owned(si.data(), P.N);
        if (P.scheme == kSchemeCKKS) {
            std::vector<client::Cplx> W, Z;
            client::build_ckks_tables(P.N, W, Z);
            W.insert(W.end(), Z.begin(), Z.begin() + P.N); // one block: W | Z
            const client::Cplx *dw = upload_owned(W.data(), 2 * P.N);
            enc_.W = dw; enc_.Z = dw + P.N;
        }
        if (!d_err_) d_err_ = upload_owned<int>(nullptr, 1);
        return enc_;
    }
    // CKKSEncoder::encode: values [n][count] (count <= N/2) at `scale` -> [n][Ltop][N] NTT-form plaintexts
    // (cplx: values [n][count][2], re then im -- he355_ckks_encode_complex, its arguments checked by cplx_args.h)
    void ckks_encode(u64 n, const double *values, u64 count, double scale, u64 *plain, bool cplx = false)
    {
        use();
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_ckks_encode needs a CKKS context");
        if (count > P.N / 2) throw std::invalid_argument("Not enough slots available to create packed plaintext");
        const EncTablesDev &T = enc_tables();
        const size_t N = P.N, L = P.Ltop;
        const u64 cmax = 256;
        u64 *zbuf = client_scratch(cmax * 2 * N);
        HIPCHECK(hipMemsetAsync(d_err_, 0, sizeof(int), stream_));
        for (u64 off = 0; off < n; off += cmax) {
            const u64 c = std::min<u64>(cmax, n - off);
            if (cplx) launch_ckks_encode_cplx(env_, c, values + off * count * 2, count, scale, zbuf, plain + off * L * N, T, d_err_);
            else launch_ckks_encode(env_, c, values + off * count, count, scale, zbuf, plain + off * L * N, T, d_err_);
            launch_ntt_forward(env_, poly_view(plain + off * L * N, (int)L, N, (int)L), (u32)c);
        }
        int err = 0;
        HIPCHECK(hipMemcpyAsync(&err, d_err_, sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        if (err) throw std::invalid_argument("encoded values are too large");
    }
    // CKKSEncoder::decode: [n][L][N] NTT-form plaintexts -> [n][total] real slot values (ranges == null: all N/2)
    // (cplx: [n][total][2], re then im -- he355_ckks_decode_complex: the same two kernels asked for no slot, then the (re, im) pairs of the
    // wanted slots gathered out of the transforms they leave in zbuf)
    void ckks_decode(int L, u64 n, const u64 *plain, double scale, double *out, const u64 *ranges = nullptr, u64 n_ranges = 0, bool cplx = false)
    {
        use();
        check_level(L);
        if (P.scheme != kSchemeCKKS) throw std::invalid_argument("he355_ckks_decode needs a CKKS context");
        if (L > 16) throw std::invalid_argument("decoding supports up to 16 data primes");
        const SlotRanges sr = slot_ranges(ranges, n_ranges, P.N / 2);
        const EncTablesDev &T = enc_tables();
        const CrtTablesDev &crt = crt_tables(L);
        const size_t N = P.N;
        const u64 cmax = 128;
        u64 *coeff = client_scratch(cmax * ((size_t)L * N + 2 * N)), *zbuf = coeff + cmax * (size_t)L * N;
        for (u64 off = 0; off < n; off += cmax) {
            const u64 c = std::min<u64>(cmax, n - off);
            HIPCHECK(hipMemcpyAsync(coeff, plain + off * L * N, c * L * N * 8, hipMemcpyDeviceToDevice, stream_));
            launch_ntt_inverse(env_, poly_view(coeff, L, N, L), (u32)c);
            if (cplx) {
                launch_ckks_decode(env_, c, coeff, scale, zbuf, out, T, crt, SlotRanges{});
                launch_ckks_gather_cplx(env_, c, zbuf, out + off * sr.total * 2, T, sr);
            } else {
                launch_ckks_decode(env_, c, coeff, scale, zbuf, out + off * sr.total, T, crt, sr);
            }
        }
        HIPCHECK(hipGetLastError());
    }
    // BatchEncoder::encode / decode: [n][count] int64 <-> [n][N] coefficients mod t
    void bfv_encode(u64 n, const long long *values, u64 count, u64 *plain)
    {
        use();
        if (t_index_ < 0) throw std::invalid_argument("he355_bfv_encode needs a BFV context with a batching plain modulus");
        if (count > P.N) throw std::invalid_argument("Not enough slots available to create packed plaintext");
        const EncTablesDev &T = enc_tables();
        HIPCHECK(hipMemsetAsync(plain, 0, n * P.N * 8, stream_));
        launch_bfv_encode_scatter(env_, n, values, count, plain, T.slot_index, P.plain_modulus);
        PolyView v = poly_view(plain, 1, P.N, 1);
        v.prime_of[0] = (unsigned char)t_index_;
        launch_ntt_inverse(env_, v, (u32)n);
        HIPCHECK(hipGetLastError());
    }
    void bfv_decode(u64 n, const u64 *plain, long long *out, const u64 *ranges = nullptr, u64 n_ranges = 0)
    {
        use();
        if (t_index_ < 0) throw std::invalid_argument("he355_bfv_decode needs a BFV context with a batching plain modulus");
        const SlotRanges sr = slot_ranges(ranges, n_ranges, P.N);
        const EncTablesDev &T = enc_tables();
        const u64 cmax = 1024;
        u64 *ev = client_scratch(cmax * P.N);
        for (u64 off = 0; off < n; off += cmax) {
            const u64 c = std::min<u64>(cmax, n - off);
            HIPCHECK(hipMemcpyAsync(ev, plain + off * P.N, c * P.N * 8, hipMemcpyDeviceToDevice, stream_));
            PolyView v = poly_view(ev, 1, P.N, 1);
            v.prime_of[0] = (unsigned char)t_index_;
            launch_ntt_forward(env_, v, (u32)c);
            launch_bfv_decode_gather(env_, c, ev, out + off * sr.total, T.slot_index, P.plain_modulus, sr);
        }
        HIPCHECK(hipGetLastError());
    }
    void ntt(u64 *polys, u64 n_polys, const uint8_t *prime_of, u32 period, bool inverse)
    {
        use();
        if (period == 0 || period > 64) throw std::invalid_argument("prime map period must be in [1, 64]");
        if (n_polys % period) throw std::invalid_argument("polynomial count must be a multiple of the prime map period");
        PolyView v;
        v.base = polys; v.item_stride = (u64)period * P.N; v.polys_per_item = (int)period; v.pad_ = 0;
        for (u32 i = 0; i < period; ++i) {
            if (prime_of[i] >= P.K + P.aux.size()) throw std::invalid_argument("prime index out of range");
            v.prime_of[i] = prime_of[i];
        }
        if (inverse) launch_ntt_inverse(env_, v, (u32)(n_polys / period));
        else launch_ntt_forward(env_, v, (u32)(n_polys / period));
        HIPCHECK(hipGetLastError());
    }
    void timer_begin()
    {
        use();
        probe_.used = 0;
        probe_.ops = 0;
        env_.probe = &probe_; // probed until timer_end
        HIPCHECK(hipEventRecord(ev0_, stream_));
    }
    // dominant-kernel probe of the region closed by the last timer_end: total duration, launches, ops covered
    void probe_result(float *total_ms, u64 *launches, u64 *ops)
    {
        use();
        float tot = 0;
        for (int i = 0; i < probe_.used; ++i) {
            float ms = 0;
            HIPCHECK(hipEventSynchronize(probe_.stop[i]));
            HIPCHECK(hipEventElapsedTime(&ms, probe_.start[i], probe_.stop[i]));
            tot += ms;
        }
        if (total_ms) *total_ms = tot;
        if (launches) *launches = (u64)probe_.used;
        if (ops) *ops = probe_.ops;
    }
    float timer_end()
    {
        use();
        HIPCHECK(hipEventRecord(ev1_, stream_));
        HIPCHECK(hipEventSynchronize(ev1_));
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, ev0_, ev1_));
        env_.probe = nullptr;
        return ms;
    }
    void sync() { use(); HIPCHECK(hipStreamSynchronize(stream_)); HIPCHECK(hipStreamSynchronize(stream2_)); }
    // clock probe: started BEFORE the region it measures (the wave takes its slot first), bounded by `duration_us` of real time
    void clock_probe_begin(u64 duration_us)
    {
        use();
        if (duration_us == 0 || duration_us > 10000000) throw std::invalid_argument("clock probe duration must be in (0, 10 s]");
        if (!probe_stream_) HIPCHECK(hipStreamCreateWithFlags(&probe_stream_, hipStreamNonBlocking));
        if (!d_clock_) d_clock_ = upload_owned<u64>(nullptr, 2);
        HIPCHECK(hipMemsetAsync(d_clock_, 0, 2 * sizeof(u64), probe_stream_));
        hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, probe_stream_, duration_us * 100, d_clock_);
        HIPCHECK(hipGetLastError());
    }
    void clock_probe_end(double *mhz, double *seconds)
    {
        use();
        if (!probe_stream_ || !d_clock_) throw std::logic_error("clock probe not started");
        u64 h[2] = {0, 0};
        HIPCHECK(hipMemcpyAsync(h, d_clock_, sizeof h, hipMemcpyDeviceToHost, probe_stream_));
        HIPCHECK(hipStreamSynchronize(probe_stream_));
        if (mhz) *mhz = h[1] ? (double)h[0] / (double)h[1] * 100.0 : 0.0;
        if (seconds) *seconds = (double)h[1] / 1e8;
    }

private:
    KernelProbe probe_;
    const Params &P;
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    KernelEnv env_{};
    PrimeDev *d_primes_ = nullptr;
    KsLimits lim_; // what the shape rules read of this context (ks_shape.h): its ring and chain, the latency / LDS limits, the chunk
    FloorConst *d_floor_ = nullptr;
    std::vector<void *> owned_;
    u64 *d_relin_ = nullptr;
    u64 *d_relin_scaled_ = nullptr; // relin_scaled()
    bool d_relin_scaled_ok_ = false;
    PrimeTables plain_tables_; // BFV: NTT tables mod t
    int t_index_ = -1;         // index of t in the device prime array (-1: none)
    EncTablesDev enc_{nullptr, nullptr, nullptr};
    int *d_err_ = nullptr;
    u64 *d_pk_ = nullptr, *d_sk_ = nullptr;
    u64 zero_seed_ = os_seed(), zero_index_ = 0;
    std::map<int, CrtTablesDev> crt_;
    std::map<int, BfvDeltaConst> bfv_delta_; // Delta_L constants per level (bfv_level_core.h)
    std::map<int, BfvNoiseConst> bfv_noise_; // t-folded CRT constants and bits(q_L) per level (bfv_noise_core.h)
    BfvDropConst *d_bfv_drop_ = nullptr;     // [Ltop][Ltop] drop-chain constants (owned_)
    std::map<uint32_t, u64 *> d_galois_;
    std::map<uint32_t, const uint32_t *> d_perm_, d_gather_; // NTT-domain permutations / coefficient-form gathers per Galois element (owned_)
    Arena arena_[kArenas];
    hipStream_t stream2_ = nullptr;
    hipStream_t probe_stream_ = nullptr; // clock_probe_begin's own stream
    u64 *d_clock_ = nullptr; // (owned_)
    hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
    bool dual_stream_ = true;
    std::map<uint32_t, std::array<unsigned char, 32>> perm_rows_;
    Counters count_;
    struct HoistKey { u64 *p = nullptr; bool ok = false; };
    std::map<uint32_t, HoistKey> d_hoist_; // hoist_key(): the permuted copies of the Galois keys, per element
    u64 cus_ = 1; // compute units of the device (the small-batch split of the modulus raise)
    bool level_walk_ = !(getenv("HE355_LEVEL_WALK") && getenv("HE355_LEVEL_WALK")[0] == '0'); // he355_rotate_sum: trie levels as grouped launches
    size_t groups_next_ = 0; // upload_groups: the next free byte of the kGroups ring
    std::map<int, BehzDev> behz_;
    DevicePool pool_;
};

} // namespace he355

// =========================================================================================================
// C ABI
// =========================================================================================================
using namespace he355;

struct he355_ctx {
    std::unique_ptr<Params> params;
    std::unique_ptr<DeviceContext> dev;
};

static thread_local std::string g_last_error;

template <class F> static int guarded(F &&f)
{
    try {
        f();
        return HE355_OK;
    } catch (const DeviceError &e) {
        g_last_error = e.what();
        return HE355_E_DEVICE;
    } catch (const std::invalid_argument &e) {
        g_last_error = e.what();
        return HE355_E_INVALID_ARGS;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return HE355_E_PARAMS;
    } catch (...) {
        g_last_error = "unknown error";
        return HE355_E_CRITICAL;
    }
}
static DeviceContext &dev(he355_ctx *c)
{
    if (!c) throw std::invalid_argument("null context");
    if (!c->dev) throw DeviceError("device not initialised: call he355_device_init first (no CPU fallback exists)");
    return *c->dev;
}
static Indexer to_ix(const he355_indexer &i)
{
    Indexer x;
    x.a_base = i.a_base; x.b_base = i.b_base; x.b1 = i.b1 ? i.b1 : 1; x.pairwise = i.pairwise; x.pad_ = 0;
    return x;
}

const he355::Params *he355_internal_params(const he355_ctx *ctx) { return ctx ? ctx->params.get() : nullptr; }

extern "C" {

const char *he355_last_error(void) { return g_last_error.c_str(); }

int he355_ctx_create(int scheme, uint64_t N, const int32_t *bit_sizes, uint64_t n, int plain_bits, int sec128, he355_ctx **out)
{
    if (!out || !bit_sizes) { g_last_error = "null argument"; return HE355_E_INVALID_ARGS; }
    *out = nullptr;
    try {
        std::unique_ptr<he355_ctx> c(new he355_ctx());
        c->params.reset(Params::create(scheme, (size_t)N, std::vector<int>(bit_sizes, bit_sizes + n), plain_bits, sec128 != 0));
        *out = c.release();
        return HE355_OK;
    } catch (const std::exception &e) { // SEAL exceptions are reported as code 2 by the reference (seal_context.cpp:94-97)
        g_last_error = e.what();
        return HE355_E_PARAMS;
    }
}
int he355_ctx_create_primes(int scheme, uint64_t N, const uint64_t *primes, uint64_t n, uint64_t plain_modulus, he355_ctx **out)
{
    if (!out || !primes) { g_last_error = "null argument"; return HE355_E_INVALID_ARGS; }
    *out = nullptr;
    try {
        std::unique_ptr<he355_ctx> c(new he355_ctx());
        c->params.reset(Params::create_primes(scheme, (size_t)N, std::vector<u64>(primes, primes + n), plain_modulus));
        *out = c.release();
        return HE355_OK;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return HE355_E_PARAMS;
    }
}
void he355_ctx_destroy(he355_ctx *ctx) { delete ctx; }
uint64_t he355_poly_degree(const he355_ctx *c) { return c->params->N; }
uint64_t he355_key_modulus_count(const he355_ctx *c) { return c->params->K; }
uint64_t he355_data_modulus_count(const he355_ctx *c) { return c->params->Ltop; }
uint64_t he355_modulus(const he355_ctx *c, uint64_t i) { return i < c->params->K ? c->params->primes[i].q : 0; }
uint64_t he355_plain_modulus(const he355_ctx *c) { return c->params->plain_modulus; }
int he355_prime_uses_fp64(const he355_ctx *c, uint64_t i) { return i < c->params->K ? (int)c->params->primes[i].f64 : 0; }
uint64_t he355_bfv_aux_base(const he355_ctx *c, int level, uint64_t *out, uint64_t cap)
{
    const Params &p = *c->params;
    if (p.scheme != kSchemeBFV || level < 1 || (size_t)level > p.Ltop) return 0;
    try {
        const size_t nB = p.behz_nB(level);
        for (size_t i = 0; i <= nB && i < cap; ++i) out[i] = p.aux[i].q;
        return nB + 1;
    } catch (const std::exception &) {
        return 0;
    }
}
uint32_t he355_galois_elt_from_step(const he355_ctx *c, int step) { return c->params->galois_elt_from_step(step); }
uint64_t he355_galois_elts_all(const he355_ctx *c, uint32_t *out, uint64_t cap)
{
    const auto v = c->params->galois_elts_all();
    for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
    return v.size();
}

int he355_device_count(int *count)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    if (e != hipSuccess) { g_last_error = std::string("HIP error: ") + hipGetErrorString(e); return HE355_E_DEVICE; }
    return HE355_OK;
}
int he355_device_init(he355_ctx *c, int device)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        c->dev.reset(new DeviceContext(*c->params, device));
    });
}
int he355_mem_info(he355_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes)
{
    return guarded([&] {
        dev(c).use();
        size_t f = 0, t = 0;
        HIPCHECK(hipMemGetInfo(&f, &t));
        if (free_bytes) *free_bytes = f;
        if (total_bytes) *total_bytes = t;
    });
}
int he355_malloc(he355_ctx *c, uint64_t bytes, void **d_ptr)
{
    return guarded([&] {
        if (!d_ptr) throw std::invalid_argument("null pointer");
        *d_ptr = dev(c).pool_alloc(bytes);
    });
}
int he355_free(he355_ctx *c, void *d_ptr)
{
    return guarded([&] {
        dev(c).pool_free(d_ptr);
    });
}
int he355_alloc_stats(he355_ctx *c, he355_alloc_stats_t *out)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        if (!c) { // process-wide totals (every context's pool)
            out->raw_mallocs = g_pool_totals.raw_mallocs; out->raw_frees = g_pool_totals.raw_frees;
            out->pool_hits = g_pool_totals.pool_hits; out->pool_misses = g_pool_totals.pool_misses;
            out->cached_bytes = out->live_bytes = 0;
            return;
        }
        const DevicePool::Stats st = dev(c).alloc_stats();
        out->raw_mallocs = st.raw_mallocs; out->raw_frees = st.raw_frees;
        out->pool_hits = st.pool_hits; out->pool_misses = st.pool_misses;
        out->cached_bytes = st.cached_bytes; out->live_bytes = st.live_bytes;
    });
}
int he355_path_stats(he355_ctx *c, he355_path_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).path_stats(reset != 0);
    });
}
int he355_bfv_route_stats(he355_ctx *c, he355_bfv_route_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).bfv_route_stats(reset != 0);
    });
}
int he355_bfv_multiply_stats(he355_ctx *c, he355_bfv_multiply_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).bfv_multiply_stats(reset != 0);
    });
}
int he355_pool_trim(he355_ctx *c, uint64_t *released_bytes)
{
    return guarded([&] {
        const size_t b = dev(c).pool_trim();
        if (released_bytes) *released_bytes = b;
    });
}
int he355_upload(he355_ctx *c, void *d_dst, const void *h_src, uint64_t bytes)
{
    return guarded([&] {
        dev(c).use();
        HIPCHECK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, dev(c).stream()));
        HIPCHECK(hipStreamSynchronize(dev(c).stream()));
    });
}
int he355_download(he355_ctx *c, void *h_dst, const void *d_src, uint64_t bytes)
{
    return guarded([&] {
        dev(c).use();
        HIPCHECK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, dev(c).stream()));
        HIPCHECK(hipStreamSynchronize(dev(c).stream()));
    });
}
int he355_copy(he355_ctx *c, void *d_dst, const void *d_src, uint64_t bytes)
{
    return guarded([&] {
        dev(c).use();
        if (bytes) HIPCHECK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, dev(c).stream()));
    });
}
int he355_copy_peer(he355_ctx *dst_ctx, void *d_dst, he355_ctx *src_ctx, const void *d_src, uint64_t bytes)
{
    return guarded([&] {
        // both contexts' streams are drained first (the source must be complete, the destination idle); the copy itself is
        // synchronous: load() / store() use it outside the timed operate()
        dev(src_ctx).sync();
        dev(dst_ctx).sync();
        dev(dst_ctx).use();
        if (bytes) HIPCHECK(hipMemcpyPeer(d_dst, dev(dst_ctx).device(), d_src, dev(src_ctx).device(), bytes));
    });
}
int he355_sync(he355_ctx *c) { return guarded([&] { dev(c).sync(); }); }
int he355_fill_uniform(he355_ctx *c, uint64_t *d_dst, uint64_t n_polys, const uint8_t *prime_of, uint32_t period, uint64_t seed)
{
    return guarded([&] { dev(c).fill_uniform(d_dst, n_polys, prime_of, period, seed); });
}
int he355_fill_uniform_at(he355_ctx *c, uint64_t *d_dst, uint64_t n_polys, const uint8_t *prime_of, uint32_t period, uint64_t seed, uint64_t first_poly)
{
    return guarded([&] { dev(c).fill_uniform(d_dst, n_polys, prime_of, period, seed, first_poly); });
}
int he355_set_dual_stream(he355_ctx *c, int on) { return guarded([&] { dev(c).set_dual_stream(on != 0); }); }
int he355_set_latency_max(he355_ctx *c, uint64_t n) { return guarded([&] { dev(c).set_latency_max(n); }); }
int he355_set_lds_max(he355_ctx *c, uint64_t n)
{
    return guarded([&] { dev(c).set_lds_max(n); });
}
int he355_set_level_walk(he355_ctx *c, int on) { return guarded([&] { dev(c).set_level_walk(on != 0); }); }
int he355_set_relin_key(he355_ctx *c, const uint64_t *h_key)
{
    return guarded([&] { dev(c).key_from_host(dev(c).relin_slot(), h_key); });
}
int he355_set_galois_key(he355_ctx *c, uint32_t elt, const uint64_t *h_key)
{
    return guarded([&] { dev(c).key_from_host(dev(c).galois_slot(elt), h_key); });
}
int he355_keygen_relin(he355_ctx *c, uint64_t seed)
{
    return guarded([&] { dev(c).key_generate(dev(c).relin_slot(), seed, 0); });
}
int he355_keygen_galois(he355_ctx *c, uint32_t galois_elt, uint64_t seed)
{
    return guarded([&] {
        if (!(galois_elt & 1) || galois_elt >= 2 * he355_poly_degree(c) || galois_elt < 3) throw std::invalid_argument("Galois element is not valid");
        dev(c).key_generate(dev(c).galois_slot(galois_elt), seed, galois_elt);
    });
}
int he355_set_relin_key_synthetic(he355_ctx *c, uint64_t seed)
{
    return guarded([&] { dev(c).key_synthetic(dev(c).relin_slot(), seed); });
}
int he355_set_galois_key_synthetic(he355_ctx *c, uint32_t elt, uint64_t seed)
{
    return guarded([&] { dev(c).key_synthetic(dev(c).galois_slot(elt), seed); });
}
int he355_add(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *a, const uint64_t *b, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { dev(c).addsub(L, size, n, a, b, to_ix(ix), out, false); });
}
int he355_sub(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *a, const uint64_t *b, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { dev(c).addsub(L, size, n, a, b, to_ix(ix), out, true); });
}
int he355_multiply(he355_ctx *c, int L, uint64_t n, const uint64_t *a, const uint64_t *b, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { dev(c).multiply(L, n, a, b, to_ix(ix), out); });
}
int he355_bfv_multiply(he355_ctx *c, int L, uint64_t n, const uint64_t *a, const uint64_t *b, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { dev(c).bfv_multiply(L, n, a, b, to_ix(ix), out); });
}
int he355_bfv_multiply_relin_accumulate(he355_ctx *c, int L, uint64_t rows, uint64_t cols, uint64_t inner, const uint64_t *a, uint64_t a_stride_i,
                                        uint64_t a_stride_k, const uint64_t *b, uint64_t b_stride_k, uint64_t b_stride_j, uint64_t *out)
{
    return guarded([&] { dev(c).bfv_multiply_relin_accumulate(L, rows, cols, inner, a, a_stride_i, a_stride_k, b, b_stride_k, b_stride_j, out); });
}
int he355_multiply_relin(he355_ctx *c, int L, uint64_t n, const uint64_t *a, const uint64_t *b, he355_indexer ix, int rescale, uint64_t *out)
{
    return guarded([&] { dev(c).multiply_relin(L, n, a, b, to_ix(ix), rescale != 0, out); });
}
int he355_multiply_plain(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, const uint64_t *pt, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { dev(c).plain_op(L, size, n, ct, pt, to_ix(ix), out, 0); });
}
int he355_add_plain(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, const uint64_t *pt, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { dev(c).plain_op(L, size, n, ct, pt, to_ix(ix), out, 1); });
}
// BFV level operations: the scheme is the context's (host side), so a CKKS context is refused before any device is asked for
static void need_bfv(const he355_ctx *c, const char *what)
{
    if (!c) throw std::invalid_argument("null context");
    if (c->params->scheme != kSchemeBFV) throw std::invalid_argument(std::string(what) + " needs a BFV context");
}
int he355_keygen_galois_seeded(he355_ctx *c, uint32_t galois_elt, uint64_t a_seed, uint64_t noise_seed, uint64_t *d_b)
{
    return guarded([&] {
        need_bfv(c, "he355_keygen_galois_seeded");
        plan_keygen_galois_seeded(*c->params, galois_elt, a_seed, noise_seed);
        dev(c).keygen_galois_seeded(galois_elt, a_seed, noise_seed, d_b);
    });
}
int he355_set_galois_key_seeded(he355_ctx *c, uint32_t galois_elt, const uint64_t *h_b, uint64_t a_seed)
{
    return guarded([&] {
        need_bfv(c, "he355_set_galois_key_seeded");
        plan_set_galois_key_seeded(*c->params, galois_elt, h_b);
        dev(c).key_from_seeded(galois_elt, h_b, a_seed);
    });
}
int he355_bfv_noise_budget(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *d_ct, int32_t *d_budget, int32_t *d_noise_bits)
{
    return guarded([&] { need_bfv(c, "he355_bfv_noise_budget"); dev(c).bfv_noise_budget(L, size, n, d_ct, d_budget, d_noise_bits); });
}
int he355_mod_switch_drop(he355_ctx *c, int L, int L_to, uint64_t n_polys, const uint64_t *in, uint64_t *out)
{
    return guarded([&] { dev(c).mod_switch_drop(L, L_to, n_polys, in, out); });
}
int he355_sum(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *in, uint64_t *out)
{
    return guarded([&] { dev(c).sum(L, size, n, in, out); });
}
int he355_multiply_accumulate(he355_ctx *c, int L, uint64_t rows, uint64_t cols, uint64_t inner, const uint64_t *a, uint64_t a_stride_i,
                              uint64_t a_stride_k, const uint64_t *b, uint64_t b_stride_k, uint64_t b_stride_j, uint64_t *out)
{
    return guarded([&] { dev(c).multiply_accumulate(L, rows, cols, inner, a, a_stride_i, a_stride_k, b, b_stride_k, b_stride_j, out); });
}
int he355_relinearize_rescale(he355_ctx *c, int L, uint64_t n, const uint64_t *ct3, uint64_t *out)
{
    return guarded([&] { dev(c).relinearize(L, n, ct3, out, true); });
}
int he355_relinearize(he355_ctx *c, int L, uint64_t n, const uint64_t *ct3, uint64_t *out)
{
    return guarded([&] { dev(c).relinearize(L, n, ct3, out); });
}
int he355_rescale(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *in, uint64_t *out)
{
    return guarded([&] { dev(c).rescale(L, size, n, in, out); });
}
int he355_apply_galois(he355_ctx *c, int L, uint64_t n, const uint64_t *in, uint32_t elt, uint64_t *out)
{
    return guarded([&] { dev(c).apply_galois(L, n, in, elt, out); });
}
int he355_rotate(he355_ctx *c, int L, uint64_t n, const uint64_t *in, int step, uint64_t *out)
{
    return guarded([&] { dev(c).rotate(L, n, in, step, out); });
}
int he355_hoist_stats(he355_ctx *c, he355_hoist_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).hoist_stats(reset != 0);
    });
}
int he355_hoist_release_keys(he355_ctx *c)
{
    return guarded([&] { dev(c).hoist_release_keys(); });
}
int he355_rotate_each(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const int32_t *steps, uint64_t *out)
{
    return guarded([&] {
        if (n && !steps) throw std::invalid_argument("rotate_each needs one step per ciphertext");
        dev(c).rotate_each(L, n, in, steps, out);
    });
}
int he355_rotate_sum(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const int32_t *steps, uint64_t n_steps, uint64_t *out, uint64_t *key_switches)
{
    return guarded([&] {
        if (n_steps && !steps) throw std::invalid_argument("rotate_sum needs the steps");
        const uint64_t k = dev(c).rotate_sum(L, n, in, steps, n_steps, out);
        if (key_switches) *key_switches = k;
    });
}
int he355_rotate_add(he355_ctx *c, int L, uint64_t n, const uint64_t *in, int step, const uint64_t *addend, uint64_t *out)
{
    return guarded([&] {
        if (!addend) throw std::invalid_argument("rotate_add needs an addend");
        dev(c).rotate(L, n, in, step, out, addend);
    });
}
int he355_encrypt_zero(he355_ctx *c, uint64_t n, uint64_t seed, uint64_t first_index, uint64_t *d_out)
{
    return guarded([&] { dev(c).encrypt(n, nullptr, seed, first_index, d_out); });
}
int he355_set_zero_stream(he355_ctx *c, uint64_t seed, uint64_t first_index)
{
    return guarded([&] { dev(c).set_zero_stream(seed, first_index); });
}
int he355_accumulate(he355_ctx *c, int L, uint64_t n, uint64_t *inout, uint64_t count, uint64_t *tmp)
{
    return guarded([&] { dev(c).accumulate(L, n, inout, count, tmp); });
}
int he355_ntt_forward(he355_ctx *c, uint64_t *polys, uint64_t n_polys, const uint8_t *prime_of, uint32_t period)
{
    return guarded([&] { dev(c).ntt(polys, n_polys, prime_of, period, false); });
}
int he355_ntt_inverse(he355_ctx *c, uint64_t *polys, uint64_t n_polys, const uint8_t *prime_of, uint32_t period)
{
    return guarded([&] { dev(c).ntt(polys, n_polys, prime_of, period, true); });
}
int he355_timer_begin(he355_ctx *c) { return guarded([&] { dev(c).timer_begin(); }); }
int he355_timer_end(he355_ctx *c, float *ms)
{
    return guarded([&] {
        const float v = dev(c).timer_end();
        if (ms) *ms = v;
    });
}
int he355_set_public_key(he355_ctx *c, const uint64_t *h_pk)
{
    return guarded([&] { dev(c).set_public_key(h_pk); });
}
int he355_set_secret_key(he355_ctx *c, const uint64_t *h_sk)
{
    return guarded([&] { dev(c).set_secret_key(h_sk); });
}
int he355_encrypt(he355_ctx *c, uint64_t n, const uint64_t *d_plain, uint64_t seed, uint64_t first_index, uint64_t *d_out)
{
    return guarded([&] { dev(c).encrypt(n, d_plain, seed, first_index, d_out); });
}
int he355_decrypt(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *d_ct, uint64_t *d_out)
{
    return guarded([&] { dev(c).decrypt(L, size, n, d_ct, d_out); });
}
int he355_ckks_encode(he355_ctx *c, uint64_t n, const double *d_values, uint64_t count, double scale, uint64_t *d_plain)
{
    return guarded([&] { dev(c).ckks_encode(n, d_values, count, scale, d_plain); });
}
int he355_ckks_decode(he355_ctx *c, int L, uint64_t n, const uint64_t *d_plain, double scale, double *d_out)
{
    return guarded([&] { dev(c).ckks_decode(L, n, d_plain, scale, d_out); });
}
int he355_bfv_encode(he355_ctx *c, uint64_t n, const int64_t *d_values, uint64_t count, uint64_t *d_plain)
{
    return guarded([&] { dev(c).bfv_encode(n, reinterpret_cast<const long long *>(d_values), count, d_plain); });
}
int he355_bfv_decode(he355_ctx *c, uint64_t n, const uint64_t *d_plain, int64_t *d_out)
{
    return guarded([&] { dev(c).bfv_decode(n, d_plain, reinterpret_cast<long long *>(d_out)); });
}
int he355_ckks_decode_slots(he355_ctx *c, int L, uint64_t n, const uint64_t *d_plain, double scale, const uint64_t *ranges, uint64_t n_ranges, double *d_out)
{
    return guarded([&] {
        if (!ranges) throw std::invalid_argument("null pointer");
        dev(c).ckks_decode(L, n, d_plain, scale, d_out, ranges, n_ranges);
    });
}
int he355_bfv_decode_slots(he355_ctx *c, uint64_t n, const uint64_t *d_plain, const uint64_t *ranges, uint64_t n_ranges, int64_t *d_out)
{
    return guarded([&] {
        if (!ranges) throw std::invalid_argument("null pointer");
        dev(c).bfv_decode(n, d_plain, reinterpret_cast<long long *>(d_out), ranges, n_ranges);
    });
}
// Page-locked host memory for the small, frequent transfers of a harness run (decode results, encode inputs): a copy to or from it is one
// DMA with no staging pass through the runtime's own pinned buffer
int he355_host_alloc(he355_ctx *c, uint64_t bytes, void **h_ptr)
{
    return guarded([&] {
        if (!h_ptr) throw std::invalid_argument("null pointer");
        dev(c).use();
        HIPCHECK(hipHostMalloc(h_ptr, bytes ? bytes : 8, hipHostMallocDefault));
    });
}
int he355_host_free(he355_ctx *c, void *h_ptr)
{
    return guarded([&] {
        dev(c).use();
        if (h_ptr) HIPCHECK(hipHostFree(h_ptr));
    });
}
int he355_probe_dominant_kernel(he355_ctx *c, float *total_ms, uint64_t *launches, uint64_t *ops)
{
    return guarded([&] {
        u64 l = 0, o = 0;
        dev(c).probe_result(total_ms, &l, &o);
        if (launches) *launches = l;
        if (ops) *ops = o;
    });
}
int he355_clock_probe_begin(he355_ctx *c, uint64_t duration_us) { return guarded([&] { dev(c).clock_probe_begin(duration_us); }); }
int he355_clock_probe_end(he355_ctx *c, double *mhz, double *seconds) { return guarded([&] { dev(c).clock_probe_end(mhz, seconds); }); }
int he355_set_chunk(he355_ctx *c, uint64_t ops)
{
    return guarded([&] { dev(c).set_chunk((size_t)ops); });
}

} // extern "C"

// the call families: launch sequences and C ABI of each, one file per family
#include "hoisted_rotations.inc"
#include "ckks_poly_raise.inc"
#include "ckks_complex.inc"
#include "ckks_eval_mod.inc"
#include "bfv_operands.inc"
#include "bfv_pir.inc"
