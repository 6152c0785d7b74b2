// dgs_preprocess.hip -- binning for the MI355X Gaussian sampler.
//
// Replaces PreprocessCUDA (sample_points.cu:38-98) and CudaSampler::Sampler::preprocess
// (sampler_impl.cu:216-330).  The reference bins Gaussians into 0.51-wide tiles and renders
// every (Gaussian, sample) pair of a tile -- 16 workgroups for a [-1,1)^2 domain.  Here the
// reference tile membership is reproduced exactly (radius, rect, torus wrap, clamp rules;
// num_rendered, radii, ranges are bit-identical), and each tile is refined into fine cells:
// a Gaussian is listed in a cell only if some sample of the cell can see a non-zero
// contribution: q = X^T A X <= 210, i.e. expf(power) != 0 in fp32, for entries the literal path
// may evaluate; q <= 176 for entries only the fast paths evaluate, whose bare v_exp_f32 returns +0
// beyond that (kQCutFast, dgs_internal.h).  Culled pairs are exactly-zero terms of this
// implementation, so the sums are unchanged.
//
// Work lists produced here (see dgs_internal.h for the layout):
//   * samples sorted by fine cell, per-cell sample ranges, forward work units (cell, 64 samples)
//   * Gaussians renumbered by spatial home cell (perm), per-cell Gaussian lists in ascending
//     internal id, backward work units (cell, 64 list entries)

#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "dgs_internal.h"
#include "dgs_radix.h"
#include "dgs_scan.h"

namespace dgs {

// ------------------------------------------------------------------------------ errors
static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }
int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}
int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return DGS_OK;
    g_last_error = std::string("HIP error ") + hipGetErrorString(e) + " at " + what;
    return DGS_ERR_HIP;
}

// ------------------------------------------------------------------------ launch hints
static std::mutex g_hint_mu;
static std::unordered_map<const void *, UnitHint> g_hints;
// the same records keyed by the sample buffer (hint_by_sbuf): a binning buffer's address is reused
// once the caller frees it, which replaces its g_hints entry while its sample buffer -- kept by the
// caller for dgs_bin_options.samples_binned -- is still alive
static std::unordered_map<const void *, UnitHint> g_shints;
static void hint_drop(UnitHint &h) {  // (under g_hint_mu)
    if (h.ref_done) (void)hipEventDestroy(h.ref_done);
    h.ref_done = nullptr;
}
void hint_put(const UnitHint &h) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    if (g_hints.size() > 4096) {
        for (auto &kv : g_hints) hint_drop(kv.second);
        g_hints.clear();
    }
    auto it = g_hints.find(h.gbuf);
    if (it != g_hints.end()) hint_drop(it->second);
    g_hints[h.gbuf] = h;
    if (g_shints.size() > 4096) g_shints.clear();
    UnitHint sh = h;
    sh.ref_done = nullptr;  // (owned by the g_hints entry)
    g_shints[h.sbuf] = sh;
}
bool hint_get(const void *gbuf, size_t gbytes, const void *sbuf, size_t sbytes, UnitHint *out) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    auto it = g_hints.find(gbuf);
    if (it == g_hints.end()) return false;
    const UnitHint &h = it->second;
    if (h.sbuf != sbuf || h.gbytes != gbytes || h.sbytes != sbytes) return false;
    *out = h;
    return true;
}

bool hint_by_sbuf(const void *sbuf, size_t sbytes, UnitHint *out) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    auto it = g_shints.find(sbuf);  // (the latest binning whose sample buffer has this address)
    if (it == g_shints.end() || it->second.sbytes != sbytes) return false;
    *out = it->second;
    return true;
}

static std::atomic<int64_t> g_internal_allocs{0};
static std::atomic<int64_t> g_sample_reuse{0};
void note_internal_alloc() { g_internal_allocs.fetch_add(1, std::memory_order_relaxed); }

// The binning's one host read-back target: 16 int64 of pinned host memory per host thread (the
// calls of one thread are sequential; kept for the thread's lifetime).  [0, 8): the totals;
// word 8: the sample and home sorts' look-back give-up words (read at the sync); word 9: the
// previous binning's entry-sort give-up word (copied at its end, checked at the next sync).
static int64_t *pinned_totals() {
    static thread_local int64_t *p = nullptr;
    if (!p) {
        if (hipHostMalloc(reinterpret_cast<void **>(&p), 128, hipHostMallocDefault) != hipSuccess) p = nullptr;
        else std::memset(p, 0, 128);
    }
    return p;
}

// The event after the copy of the previous binning's entry-sort give-up word into pinned word 9
// (per host thread, like the buffer): that binning may have run on another stream, so the next
// binning waits for the copy itself before reading and clearing the word.
static hipEvent_t &giveup_copied() {
    static thread_local hipEvent_t e = nullptr;
    return e;
}

static int bit_length(uint64_t v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b < 1 ? 1 : b;
}

// ------------------------------------------------------------------------- tile grid
// sample_points.cu:70-74 with torch's CUDA arithmetic (division by a CPU scalar is a
// multiplication by the float reciprocal in ATen's div_true_kernel_cuda).
__global__ void k_bounds_partial(int N, int D, const float *__restrict__ s, float *part) {
    __shared__ float smin[2][kBlock], smax[2][kBlock];
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N;
         i += (int64_t)gridDim.x * blockDim.x)
        for (int d = 0; d < D; ++d) {
            const float v = s[i * D + d];
            mn[d] = fminf(mn[d], v);
            mx[d] = fmaxf(mx[d], v);
        }
    for (int d = 0; d < 2; ++d) { smin[d][threadIdx.x] = mn[d]; smax[d][threadIdx.x] = mx[d]; }
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int d = 0; d < 2; ++d) {
                smin[d][threadIdx.x] = fminf(smin[d][threadIdx.x], smin[d][threadIdx.x + st]);
                smax[d][threadIdx.x] = fmaxf(smax[d][threadIdx.x], smax[d][threadIdx.x + st]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int d = 0; d < 2; ++d) {
            part[blockIdx.x * 4 + d] = smin[d][0];
            part[blockIdx.x * 4 + 2 + d] = smax[d][0];
        }
}

// One block (kBlock threads): tree-reduce the partial bounds, then thread 0 applies the
// reference formula.  (A single thread walking 1024 partials took ~170 us.)
__global__ __launch_bounds__(kBlock) void k_bounds_final(int nparts, int D, const float *part, int *grid, float *off) {
    __shared__ float smin[2][kBlock], smax[2][kBlock];
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int p = threadIdx.x; p < nparts; p += blockDim.x)
        for (int d = 0; d < 2; ++d) {
            mn[d] = fminf(mn[d], part[p * 4 + d]);
            mx[d] = fmaxf(mx[d], part[p * 4 + 2 + d]);
        }
    for (int d = 0; d < 2; ++d) { smin[d][threadIdx.x] = mn[d]; smax[d][threadIdx.x] = mx[d]; }
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int d = 0; d < 2; ++d) {
                smin[d][threadIdx.x] = fminf(smin[d][threadIdx.x], smin[d][threadIdx.x + st]);
                smax[d][threadIdx.x] = fmaxf(smax[d][threadIdx.x], smax[d][threadIdx.x + st]);
            }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    for (int d = 0; d < D; ++d) {
        const float ext = radd(rsub(smax[d][0], smin[d][0]), 1e-6f);
        const float inv = rdiv(1.0f, kTile);
        grid[d] = (int)ceilf(rmul(ext, inv));
        off[d] = smin[d][0];
    }
}

// ---------------------------------------------------------------------- sample binning
// Per-block tile histograms in LDS (a [-1,1)^2 domain has 16 tiles: global atomics on 16
// words serialise), flushed with one atomic per non-empty bin.
constexpr int kHistBins = 4096;
constexpr int64_t kHistGrid = 1024;  // blocks of the histogram kernels (4 per CU)
static inline unsigned hist_grid(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kHistGrid));
}

// Same-address global atomics: one word sustains ~88 atomic ops per us (MI355X_MICROARCH.md,
// 'dequeue'), so a counter that every wave or block of a large grid adds to (k_fine_count's
// largest reach: 15.6k waves, 180 us) is kept in kShards copies, one per XCD (block b adds to
// copy b % 8, its own lines), and the reader sums or maxes the copies.
constexpr int kShards = 8;
constexpr int kShard64 = 16, kShard32 = 32;  // copy strides in u64 / u32 words: 128 bytes (a line) per copy
__device__ __forceinline__ int shard_of_block() { return (int)(blockIdx.x & (kShards - 1)); }

// The digit histograms of a radix sort of the keys a producer kernel writes (dgs_radix.h's
// k_rs_hist folded into the producer: one launch less per sort).  Per block in LDS, flushed once.
struct RsHist {
    uint32_t *g;  // global [places][256] (zero-filled), null: no histogram
    int places;
};
static inline RsHist radix_hist(const RadixPlan &p, char *scratch) {  // (the plan's histograms)
    return RsHist{p.places <= 4 ? reinterpret_cast<uint32_t *>(scratch) : nullptr, p.places};
}
__device__ __forceinline__ void rs_hist_zero(uint32_t *h, const RsHist &r) {
    if (r.g)
        for (int i = threadIdx.x; i < r.places * kRsBins; i += blockDim.x) h[i] = 0u;
}
__device__ __forceinline__ void rs_hist_add(uint32_t *h, const RsHist &r, uint32_t key) {
    if (r.g)
        for (int p = 0; p < r.places; ++p) atomicAdd(&h[p * kRsBins + rs_digit(key, p * kRsBits)], 1u);
}
__device__ __forceinline__ void rs_hist_flush(const uint32_t *h, const RsHist &r) {
    if (r.g) {
        uint32_t *g = r.g + (size_t)shard_of_block() * r.places * kRsBins;  // (dgs_radix.h: kRsHistCopies)
        for (int i = threadIdx.x; i < r.places * kRsBins; i += blockDim.x)
            if (h[i]) atomicAdd(&g[i], h[i]);
    }
}

__global__ void k_sample_cells(int N, Geom G, const float *__restrict__ samples,
                               uint32_t *__restrict__ keys, uint32_t *__restrict__ ids,
                               uint32_t *__restrict__ tile_count, RsHist rh) {
    // grid-strided over a capped grid (kHistGrid blocks): the per-block LDS tile histogram is
    // flushed once, so the global same-address atomics on the few tile counters stay few
    __shared__ uint32_t hist[kHistBins];
    __shared__ uint32_t dh[4 * kRsBins];
    const bool lds = G.T <= kHistBins;
    if (lds)
        for (int t = threadIdx.x; t < G.T; t += blockDim.x) hist[t] = 0;
    rs_hist_zero(dh, rh);
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N;
         i += (int64_t)gridDim.x * blockDim.x) {
        float s[2] = {samples[i * G.D], G.D == 2 ? samples[i * G.D + 1] : 0.0f};
        const uint32_t key = ref_sample_key(G.D, s, G.grid, G.off);
        if (key < (uint32_t)G.T) {
            if (lds) atomicAdd(&hist[key], 1u);
            else atomicAdd(&tile_count[(size_t)shard_of_block() * (G.T + 1) + key], 1u);
        }
        const uint32_t ck = sample_cell_sub(G, s);  // (cell, sub-cell): cell ranges are keys >> 2
        keys[i] = ck;
        ids[i] = (uint32_t)i;
        rs_hist_add(dh, rh, ck);
    }
    __syncthreads();
    if (lds)  // (tile_count: kShards copies of T + 1 words)
        for (int t = threadIdx.x; t < G.T; t += blockDim.x)
            if (hist[t]) atomicAdd(&tile_count[(size_t)shard_of_block() * (G.T + 1) + t], hist[t]);
    rs_hist_flush(dh, rh);
}

// identifyTileRanges (sampler_impl.cu:134-151) over sorted cell keys; keys >= limit ignored.
// A second range set (beg2 non-null) over the same keys at another shift in the same launch
// (the samples' cells and sub-cells).
template <typename KT>
__global__ void k_identify(int64_t L, const KT *__restrict__ keys, uint32_t limit,
                           int32_t *__restrict__ beg, int32_t *__restrict__ end, int shift,
                           uint32_t limit2 = 0, int32_t *__restrict__ beg2 = nullptr,
                           int32_t *__restrict__ end2 = nullptr, int shift2 = 0,
                           const int64_t *__restrict__ Ldev = nullptr) {
    if (Ldev) L = min(L, max(sload(Ldev), (int64_t)0));  // (a capacity-sized launch: the device count)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const uint32_t kr = (uint32_t)keys[i], pr = i > 0 ? (uint32_t)keys[i - 1] : 0u;
#pragma unroll
    for (int set = 0; set < 2; ++set) {
        if (set == 1 && !beg2) break;
        const int sh = set ? shift2 : shift;
        const uint32_t lim = set ? limit2 : limit;
        int32_t *b = set ? beg2 : beg, *e = set ? end2 : end;
        const uint32_t k = kr >> sh;
        if (i == 0) {
            if (k < lim) b[k] = 0;
        } else {
            const uint32_t p = pr >> sh;
            if (k != p) {
                if (p < lim) e[p] = (int32_t)i;
                if (k < lim) b[k] = (int32_t)i;
            }
        }
        if (i == L - 1 && k < lim) e[k] = (int32_t)L;
    }
}

// ------------------------------------------------------------------- Gaussian binning
// A Gaussian's reference rect (ref_key_rect) as four int16 in two words, computed once by
// k_gauss_prep; a rect that does not fit int16 is stored as kRectNone and recomputed.
constexpr uint32_t kRectNone = 0x80008000u;
__device__ __forceinline__ uint2 rect_pack(const KeyRect &k) {
    const bool fits = k.x0 > -32768 && k.x0 < 32768 && k.x1 > -32768 && k.x1 < 32768 && k.y0 > -32768 &&
                      k.y0 < 32768 && k.y1 > -32768 && k.y1 < 32768;
    if (!fits) return make_uint2(kRectNone, kRectNone);
    return make_uint2(((uint32_t)k.x0 & 0xffffu) | ((uint32_t)k.x1 << 16), ((uint32_t)k.y0 & 0xffffu) | ((uint32_t)k.y1 << 16));
}
__device__ __forceinline__ KeyRect rect_get(uint2 p, int D, const float *m, float r, const Geom &G) {
    if (p.x == kRectNone) return ref_key_rect(D, m, r, G.grid, G.off);
    KeyRect k;
    k.x0 = (int)(int16_t)(p.x & 0xffffu);
    k.x1 = (int)(int16_t)(p.x >> 16);
    k.y0 = (int)(int16_t)(p.y & 0xffffu);
    k.y1 = (int)(int16_t)(p.y >> 16);
    return k;
}

// forward.cu:24-83 (radius, tiles touched) + the reference tile counts + spatial home key.
// Also packs each Gaussian's mean, radius and conic into one 32-byte record (caller order,
// coalesced): k_fine_count then gathers one record per Gaussian in internal order instead of
// three scattered arrays.
__global__ void k_gauss_prep(int P, Geom G, const float *__restrict__ means,
                             const float *__restrict__ covs, const float *__restrict__ conics,
                             float *__restrict__ radii,
                             uint64_t *__restrict__ touched, uint32_t *__restrict__ tile_count,
                             uint32_t *__restrict__ home, uint32_t *__restrict__ ids,
                             int home_w, int home_h, const uint8_t *__restrict__ present,
                             float4 *__restrict__ grec, RsHist rh) {
    __shared__ uint32_t hist[kHistBins];  // grid-strided, capped grid: see k_sample_cells
    __shared__ uint32_t dh[4 * kRsBins];  // (the home sort's digit counts)
    const bool lds = G.T <= kHistBins;
    if (lds)
        for (int t = threadIdx.x; t < G.T; t += blockDim.x) hist[t] = 0;
    rs_hist_zero(dh, rh);
    __syncthreads();
    const int D = G.D, S = D * (D + 1) / 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P;
         i += (int64_t)gridDim.x * blockDim.x) {
        float r = 0.0f;
        float m[2] = {means[i * D], D == 2 ? means[i * D + 1] : 0.0f};
        float cv[3] = {covs[i * S], D == 2 ? covs[i * S + 1] : 0.0f, D == 2 ? covs[i * S + 2] : 0.0f};
        uint32_t t = ref_touched(D, m, cv, G.grid, G.off, &r);
        if (present && !present[i]) {  // left out of this binning, as a det == 0 Gaussian is
            r = 0.0f;
            t = 0u;
        }
        radii[i] = r;
        touched[i] = t;
        ids[i] = (uint32_t)i;
        const KeyRect kr = ref_key_rect(D, m, r, G.grid, G.off);
        {
            const float c0 = conics[i * S], c1 = D == 2 ? conics[i * S + 1] : 0.0f;
            const float c2 = D == 2 ? conics[i * S + 2] : 0.0f;
            const uint2 pk = rect_pack(kr);  // (k_fine_count / k_fine_fill reuse the rect)
            grec[2 * i] = make_float4(m[0], m[1], r, c0);
            grec[2 * i + 1] = make_float4(c1, c2, __uint_as_float(pk.x), __uint_as_float(pk.y));
        }
        if (!(r > 0.0f)) {
            home[i] = (uint32_t)home_w * (uint32_t)home_h;  // absent: after every home cell
            rs_hist_add(dh, rh, (uint32_t)home_w * (uint32_t)home_h);
            continue;
        }
        for (int y = kr.y0; y < kr.y1; ++y)
            for (int x = kr.x0; x < kr.x1; ++x) {
                const uint32_t key = key_of(D, x, y, G.grid);
                if (key < (uint32_t)G.T) {
                    if (lds) atomicAdd(&hist[key], 1u);
                    else atomicAdd(&tile_count[(size_t)shard_of_block() * (G.T + 1) + key], 1u);
                }
            }
        int h[2] = {0, 0};
        const int lim[2] = {home_w, home_h};
        for (int d = 0; d < D; ++d) {
            const double u = ((double)m[d] - (double)G.off[d]) * G.ifs;
            int v = (u == u) ? (int)floor(fmin(fmax(u, -1.0), (double)lim[d])) : 0;
            h[d] = v < 0 ? 0 : (v >= lim[d] ? lim[d] - 1 : v);
        }
        home[i] = (uint32_t)(h[1] * home_w + h[0]);
        rs_hist_add(dh, rh, (uint32_t)(h[1] * home_w + h[0]));
    }
    __syncthreads();
    if (lds)  // (tile_count: kShards copies of T + 1 words)
        for (int t = threadIdx.x; t < G.T; t += blockDim.x)
            if (hist[t]) atomicAdd(&tile_count[(size_t)shard_of_block() * (G.T + 1) + t], hist[t]);
    rs_hist_flush(dh, rh);
}

// Does [xa, xb] x [ya, yb] contain an X with X^T A X <= qcut?  (convex quadratic: the
// minimum over a box is at the origin if inside, else on an edge at the clamped critical point)
__device__ inline bool box_hits_ellipse(double xa, double xb, double ya, double yb, double c0,
                                        double c1, double c2, double qcut) {
    if (xa <= 0.0 && xb >= 0.0 && ya <= 0.0 && yb >= 0.0) return true;
    double best = INFINITY;
    const double xs[2] = {xa, xb}, ys[2] = {ya, yb};
    for (int k = 0; k < 2; ++k) {
        const double x = xs[k];
        const double y = fmin(fmax(-c1 * x / c2, ya), yb);
        best = fmin(best, c0 * x * x + 2.0 * c1 * x * y + c2 * y * y);
        const double yy = ys[k];
        const double xx = fmin(fmax(-c1 * yy / c0, xa), xb);
        best = fmin(best, c0 * xx * xx + 2.0 * c1 * xx * yy + c2 * yy * yy);
    }
    return best <= qcut * (1.0 + 1e-6) + 1e-12;
}

#ifndef DGS_CUT_EXACT
#define DGS_CUT_EXACT 1
#endif
#if DGS_CUT_EXACT
#define DGS_CUT_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DGS_CUT_CONTRACT
#endif
// ---- the cut geometry of one Gaussian, shared by the per-Gaussian enumeration (enumerate_fine,
// the sort path) and the per-cell gather (k_gather): both must take the same decisions bit for
// bit, so these helpers run with contraction off.
struct Cut {
    // e: half-widths of the reference cut kQCut (eligibility, shifted images, anything that may
    // become kUnsafe); ef: those of the fast cut G.qf, for visits whose entries only the fast
    // paths evaluate (enumerate_fine's `fast` visits, local_rows); ef <= e, and ef == e bit for bit when G.qf == kQCut
    double e[2], ef[2], md[2], epsx[2], c0, c1, c2;
    bool pd, cull;
};

__device__ __forceinline__ Cut gauss_cut(const Geom &G, const float *m, const float *con) {
    DGS_CUT_CONTRACT
    const int D = G.D;
    Cut k;
    k.c0 = con[0];
    k.c1 = D == 2 ? con[1] : 0.0;
    k.c2 = D == 2 ? con[2] : 0.0;
    k.e[0] = k.e[1] = INFINITY;
    if (D == 1) {
        k.pd = k.c0 > 0.0 && k.c0 < INFINITY;
        if (k.pd) k.e[0] = sqrt(kQCut / k.c0) * (1.0 + 1e-6);
    } else {
        const double det = k.c0 * k.c2 - k.c1 * k.c1;
        // (past kRho2Max the fp32 exponent's rounding is amplified beyond the cut's margin:
        // such conics keep their whole tiles, like the non-PD ones)
        k.pd = k.c0 > 0.0 && det > 0.0 && det < INFINITY && k.c0 < INFINITY && k.c2 < INFINITY &&
               k.c1 * k.c1 < kRho2Max * (k.c0 * k.c2);
        if (k.pd) {
            k.e[0] = sqrt(kQCut * k.c2 / det) * (1.0 + 1e-6);
            k.e[1] = sqrt(kQCut * k.c0 / det) * (1.0 + 1e-6);
        }
    }
    k.cull = k.pd && k.e[0] < 0.5 && (D == 1 || k.e[1] < 0.5);
    k.ef[0] = k.e[0] * G.rf;
    k.ef[1] = k.e[1] * G.rf;
    for (int d = 0; d < 2; ++d) {
        k.md[d] = d < D ? (double)m[d] - (double)G.off[d] : 0.0;
        k.epsx[d] = 1e-6 * (1.0 + fabs((double)m[d]) + fabs((double)G.off[d]));
    }
    return k;
}

// One axis of a tile visit: the torus shift ks and the fine-index range [flo, fhi] the cut can
// reach in tile coordinate tcd; false if none.
__device__ __forceinline__ bool axis_setup(const Geom &G, const Cut &k, int d, int tcd, int &ks, int &flo, int &fhi) {
    DGS_CUT_CONTRACT
    ks = 0;
    if (!k.cull) {
        flo = 0;
        fhi = G.n - 1;
        return true;
    }
    const double BS = (double)kTile, slack = kCellSlack * G.fs;
    const double o = tcd * BS;
    const double xa = k.md[d] - (o + BS + slack) - k.epsx[d];
    const double xb = k.md[d] - (o - slack) + k.epsx[d];
    const double klo = ceil((xa - k.e[d]) * 0.5), khi = floor((xb + k.e[d]) * 0.5);
    if (klo > khi) return false;
    ks = (int)klo;  // e < 0.5 and a tile narrower than 1: at most one k
    const double dl = k.md[d] - 2.0 * klo - k.e[d] - k.epsx[d];
    const double dh = k.md[d] - 2.0 * klo + k.e[d] + k.epsx[d];
    const int lo = (int)floor(fmax((dl - o) * G.ifs - kCellSlack, -1.0));
    const int hi = (int)floor(fmin((dh - o) * G.ifs + kCellSlack, (double)G.n));
    flo = lo < 0 ? 0 : lo;
    fhi = hi > G.n - 1 ? G.n - 1 : hi;
    return flo <= fhi;
}

// A local visit (visit_local: the k = 0 image, |X| < 1 in every cell it meets) of a conic that is
// not kUnsafe emits flag-free entries only -- evaluated by the fast paths alone, whose G is a
// hardware zero beyond G.qf (dgs_internal.h, kQCutFast): its cells are those of the fast cut.
// Narrows axis d's range [flo, fhi] of axis_setup (ks = 0) to it; false if none is left.
__device__ __forceinline__ bool axis_fast(const Geom &G, const Cut &k, int d, int tcd, int &flo, int &fhi) {
    DGS_CUT_CONTRACT
    const double o = tcd * (double)kTile;
    const double dl = k.md[d] - k.ef[d] - k.epsx[d];
    const double dh = k.md[d] + k.ef[d] + k.epsx[d];
    const int lo = (int)floor(fmax((dl - o) * G.ifs - kCellSlack, -1.0));
    const int hi = (int)floor(fmin((dh - o) * G.ifs + kCellSlack, (double)G.n));
    flo = max(flo, lo);
    fhi = min(fhi, hi);
    return flo <= fhi;
}

// The row's cells that meet the ellipse X^T A X <= q (D = 2, culled): project the ellipse's
// slice over the row's X1 band onto X0 (a slice of a convex set is convex, so "box meets
// ellipse" <=> the cell's X0 range meets that interval), in fp32 with local_rows' construction
// and margins: the slice ends' fp32 error is at most ~sqrt(8 eps) e0 sqrt(1 - rho^2) where the
// sqrt argument cancels (the ellipse's top and bottom), so tol = 2e-3 e0 + 1e-5 (|xl| + |xu|) in
// displacement units, and 1e-4 of a cell on the cell index.  An extra candidate only evaluates
// exact zeros.  (The fp64 form -- a division and two square roots per row, det and e0 per row --
// was most of k_fine_count_irr's and k_fine_fill's issue slots in thin fields, whose sort path
// holds three quarters of the entries.)  Per Gaussian init(); per row cols() narrows [fxl, fxh]
// for the visit whose tile-relative mean (torus shift included) is (md0, md1).
struct Slice32 {
    // (r*: the reference cut kQCut; f*: the fast cut G.qf of fast-path-only visits)
    float rqcc0, ryu0, re1, rtol0, fqcc0, fyu0, fe1, ftol0;
    float c1, det, ic0, eps0, eps1, fs, ifs, slack;
    __device__ __forceinline__ void init(const Geom &G, const Cut &k) {
        const float qc = (float)(kQCut * (1.0 + 1e-6)), qcf = (float)(G.qf * (1.0 + 1e-6));
        const float c0f = (float)k.c0, c2f = (float)k.c2, e0 = (float)k.e[0], e0f = (float)k.ef[0];
        c1 = (float)k.c1;
        det = (float)(k.c0 * k.c2 - k.c1 * k.c1);
        ic0 = 1.0f / c0f;
        ryu0 = -c1 * e0 / c2f;
        fyu0 = -c1 * e0f / c2f;
        rqcc0 = qc * c0f;
        fqcc0 = qcf * c0f;
        re1 = (float)k.e[1];
        fe1 = (float)k.ef[1];
        eps0 = (float)k.epsx[0] + 1e-6f;
        eps1 = (float)k.epsx[1] + 1e-6f;
        rtol0 = 2e-3f * e0 + 1e-5f;
        ftol0 = 2e-3f * e0f + 1e-5f;
        fs = (float)G.fs;
        ifs = (float)G.ifs;
        slack = (float)(kCellSlack * G.fs);
    }
    __device__ __forceinline__ bool cols(int fy, float md0, float md1, int n, int &fxl, int &fxh, bool fast) const {
        const float qcc0 = fast ? fqcc0 : rqcc0, yu0 = fast ? fyu0 : ryu0, yl0 = -yu0;
        const float e1 = fast ? fe1 : re1, tol0 = fast ? ftol0 : rtol0;
        const float ya = fmaxf(md1 - ((float)(fy + 1) * fs + slack) - eps1, -e1);
        const float yb = fminf(md1 - ((float)fy * fs - slack) + eps1, e1);
        if (!(ya <= yb)) return false;
        const float yu = fminf(fmaxf(yu0, ya), yb), yl = fminf(fmaxf(yl0, ya), yb);
        // (v_sqrt_f32, ~1 ulp: far inside tol)
        const float xu = (-c1 * yu + __builtin_amdgcn_sqrtf(fmaxf(qcc0 - det * yu * yu, 0.0f))) * ic0;
        const float xl = (-c1 * yl - __builtin_amdgcn_sqrtf(fmaxf(qcc0 - det * yl * yl, 0.0f))) * ic0;
        const float tol = tol0 + 1e-5f * (fabsf(xu) + fabsf(xl));
        const float fa = ceilf((md0 - slack - eps0 - (xu + tol)) * ifs - 1.0f - 1e-4f);
        const float fb = floorf((md0 + slack + eps0 - (xl - tol)) * ifs + 1e-4f);
        fxl = max(fxl, (int)fminf(fmaxf(fa, -1.0f), (float)n));
        fxh = min(fxh, (int)fmaxf(fminf(fb, (float)n), -1.0f));
        return true;
    }
};

// A tile visit is `local` when the cut reaches it unshifted (ks = 0) and stays well inside one
// period, so every cell it meets holds |X| < 1 (no wrap, no sample-box test).
__device__ __forceinline__ bool visit_local(const Geom &G, const Cut &k, const int *ks) {
    return k.cull && ks[0] == 0 && ks[1] == 0 && k.e[0] + 3.0 * G.fs < 0.9 &&
           (G.D == 1 || k.e[1] + 3.0 * G.fs < 0.9);
}

// Gather-path Gaussians ("regular"): D = 2, culled, well-conditioned, its mean inside the fine
// grid and its cut within kGatherReach fine cells of the mean's (home) cell.  Their local
// entries are produced per cell by k_gather (no sort); everything else goes through the
// per-Gaussian enumeration and the entry sort.  Returns the reach in cells, 0 if not regular.
// Thin conics (rho^2 >= 0.82) are regular too: local_rows' fp32 slice margins hold for them -- the slice centre's rounding is relative
// to |x|, and the sqrt argument's cancellation costs at most sqrt(eps) e0 sqrt(1 - rho^2) <= tol
// (rho^2 < kRho2Max keeps det well away from 0).
#ifndef DGS_THIN_GATHER
#define DGS_THIN_GATHER 1
#endif
#ifndef DGS_GATHER_REACH
#define DGS_GATHER_REACH 6
#endif
constexpr int kGatherReach = DGS_GATHER_REACH, kGatherRows = 2 * kGatherReach + 1;
static_assert(kGatherRows <= 32, "local_rows keeps one bit per row");
__device__ __forceinline__ int gather_reach(const Geom &G, const float *m, float r, const float *con, const Cut &k,
                                            const KeyRect &kr) {
    if (G.D != 2 || !(r > 0.0f) || !k.cull || conic_unsafe(2, con[0], con[1], con[2]) ||
        (!DGS_THIN_GATHER && conic_thin(2, con[0], con[1], con[2])))
        return 0;
    if (!(k.e[0] + 3.0 * G.fs < 0.9 && k.e[1] + 3.0 * G.fs < 0.9)) return 0;
    // every tile visited at most once (a rect wider than the grid visits a tile repeatedly,
    // which the enumeration reproduces entry by entry); kr = ref_key_rect(2, m, r, ...)
    if (kr.x1 - kr.x0 > G.grid[0] || kr.y1 - kr.y0 > G.grid[1]) return 0;
    const int lim[2] = {G.grid[0] * G.n, G.grid[1] * G.n};
    int reach = 0;
    for (int d = 0; d < 2; ++d) {
        const double u = ((double)m[d] - (double)G.off[d]) * G.ifs;
        if (!(u >= 0.0 && u < (double)lim[d])) return 0;  // (the home cell is clamped)
        reach = max(reach, (int)ceil(k.e[d] * G.ifs + 2.0));
    }
    return reach <= kGatherReach ? reach : 0;
}

// Unculled Gaussians take k_wide (one wave per Gaussian) instead of enumerate_fine.
__device__ __forceinline__ bool wide_gauss(const Cut &k) { return !k.cull; }
constexpr unsigned kWideBlocks = 128;  // (grid-strided over the device-side queue length)

// Enumerate the fine entries (cell, id|flag) of one Gaussian, in the reference's tile-key
// order (sampler_impl.cu:94-124), restricted to non-empty cells that pass the exact cull.
// skip_local: leave out the cells of the direct local tile visits (a regular Gaussian's:
// k_gather makes them).
// Per tile, whether its fallback cell holds samples: bits of fbg (set by k_sub_box /
// k_cell_box, one word per 32 tiles).  The first 64 tiles' bits are preloaded into registers
// (scalar loads, no LDS pass and no barrier: the usual grids have 4 x 4 tiles); later tiles
// read fbg through the cache.
struct FbBits {
    uint64_t w;
    const uint32_t *g;
    __device__ __forceinline__ bool full(uint32_t key) const {
        return key < 64u ? ((w >> key) & 1ull) != 0ull : ((g[key >> 5] >> (key & 31)) & 1u) != 0u;
    }
};
__device__ __forceinline__ FbBits fb_load(const uint32_t *__restrict__ fbg, int T) {
    FbBits b;
    b.g = fbg;
    const uint32_t lo = sload(&fbg[0]), hi = T > 32 ? sload(&fbg[1]) : 0u;
    b.w = (uint64_t)lo | ((uint64_t)hi << 32);
    return b;
}

template <class Emit>
__device__ __forceinline__ void enumerate_fine(const Geom &G, const float *m, float r, const float *con, const Cut &k,
                                      bool skip_local, const int32_t *__restrict__ sbeg,
                                      const int32_t *__restrict__ send,
                                      const float4 *__restrict__ box, const FbBits &fbits, uint32_t id,
                                      Emit emit) {
    const int D = G.D;
    const KeyRect kr = ref_key_rect(D, m, r, G.grid, G.off);
    const uint32_t uflag = conic_unsafe(D, con[0], con[1], con[2]) ? kUnsafe : 0u;
    Slice32 sl;
    if (k.cull && D == 2) sl.init(G, k);
    for (int y = kr.y0; y < kr.y1; ++y)
        for (int x = kr.x0; x < kr.x1; ++x) {
            const uint32_t key = key_of(D, x, y, G.grid);
            if (key >= (uint32_t)G.T) continue;
            const int tc[2] = {D == 1 ? (int)key : (int)(key % (uint32_t)G.grid[0]),
                               D == 1 ? 0 : (int)(key / (uint32_t)G.grid[0])};
            const uint32_t base = key * (uint32_t)G.CT;
            int flo[2] = {0, 0}, fhi[2] = {0, 0}, ks[2] = {0, 0};
            // (both axes spelled out: with a loop over d the Cut's per-axis arrays were indexed
            // dynamically, from scratch memory, on every tile visit)
            bool any = axis_setup(G, k, 0, tc[0], ks[0], flo[0], fhi[0]);
            if (any && D == 2) any = axis_setup(G, k, 1, tc[1], ks[1], flo[1], fhi[1]);
            const bool local = visit_local(G, k, ks);
            // (entries of such a visit are flag-free: only the fast paths evaluate them)
            const bool fast = local && !uflag;
            if (any && fast) {
                any = axis_fast(G, k, 0, tc[0], flo[0], fhi[0]);
                if (any && D == 2) any = axis_fast(G, k, 1, tc[1], flo[1], fhi[1]);
            }
            // (k_gather makes the direct -- unwrapped -- local visits of a regular Gaussian)
            const bool direct = x >= 0 && x < G.grid[0] && (D == 1 || (y >= 0 && y < G.grid[1]));
            if (any && !(skip_local && local && direct)) {
                const int ylo = D == 2 ? flo[1] : 0, yhi = D == 2 ? fhi[1] : 0;
                // (the visit's tile-relative mean, torus shift included: |md| < 2, so the fp32
                // rounding is far inside eps0 / eps1)
                const float md0 = (float)(k.md[0] - tc[0] * (double)kTile - 2.0 * ks[0]);
                const float md1 = (float)(k.md[1] - tc[1] * (double)kTile - 2.0 * ks[1]);
                for (int fy = ylo; fy <= yhi; ++fy) {
                    int fxl = flo[0], fxh = fhi[0];
                    if (k.cull && D == 2 && !sl.cols(fy, md0, md1, G.n, fxl, fxh, fast)) continue;
                    for (int fx = fxl; fx <= fxh; ++fx) {
                        const uint32_t cell = base + (uint32_t)(fy * G.n + fx);
                        // Empty cells get no units: an entry there would never be read, and its
                        // backward slot (k_bwd_esum sums every slot of a Gaussian) never written.
                        if (send[cell] <= sbeg[cell]) continue;
                        if (k.cull && D == 1) {
                            const double slack = kCellSlack * G.fs;
                            const double o = tc[0] * (double)kTile;
                            const double dlo = o + fx * G.fs - slack, dhi = o + (fx + 1) * G.fs + slack;
                            const double xa = k.md[0] - dhi - k.epsx[0], xb = k.md[0] - dlo + k.epsx[0];
                            const double ee = fast ? k.ef[0] : k.e[0];
                            if (!(xa - 2.0 * ks[0] <= ee && xb - 2.0 * ks[0] >= -ee)) continue;
                        }
                        // Wrap class from the cell's actual samples (box = their bounding box;
                        // the nominal cell may reach past the last sample): kGeneral when some
                        // |X| may exceed 1 (torus wrap) -- a constant shift over the cell unless
                        // the X range crosses a wrap breakpoint, which takes the fully general
                        // per-pair path (kUnsafe).  eps covers the float rounding of m - s.
                        // Unshifted (k = 0) cells of a culled Gaussian lie within e + fs of its
                        // mean, so |X| < 1 there whenever e + fs stays well below 1.
                        uint32_t cls = 0u;
                        if (!local) {
                            const float4 bx = box[cell];
                            const double blo[2] = {bx.x, bx.y}, bhi[2] = {bx.z, bx.w};
                            bool inside = true, constant = true;
#pragma unroll
                            for (int d = 0; d < 2; ++d) {
                                if (d >= D) break;
                                const double eps = 1e-6 * (1.0 + fabs((double)m[d]) + fmax(fabs(blo[d]), fabs(bhi[d])));
                                const double wa = (double)m[d] - bhi[d] - eps, wb = (double)m[d] - blo[d] + eps;
                                inside = inside && wa >= -1.0 && wb <= 1.0;
                                constant = constant && wrap_shift(wa) == wrap_shift(wb);
                            }
                            cls = inside ? 0u : (constant ? kGeneral : kGeneral | kUnsafe);
                        }
                        emit(cell, id | uflag | cls);
                    }
                }
            }
            if (fbits.full(key)) emit(base + (uint32_t)(G.CT - 1), id | kUnsafe | kGeneral);  // whole tile: general path
        }
}

// enumerate_fine for a regular (gather-path) Gaussian whose reference rect lies inside the grid
// (no wrapped tile keys): every visit is direct and local -- k_gather makes its cells -- so the
// enumeration emits only the fallback cells of its tiles (in the same tile order).  Returns
// false when the rect is not inside (then enumerate_fine runs).  The cut of a regular Gaussian
// reaches no torus image of a tile within its rect (e < 0.5 while an image is 2 away), which is
// why no tile of an inside rect has a shifted visit.
template <class Emit>
__device__ __forceinline__ bool fallback_only(const Geom &G, const KeyRect &kr, const FbBits &fbits, uint32_t id,
                                              Emit emit) {
    if (kr.x0 < 0 || kr.y0 < 0 || kr.x1 > G.grid[0] || kr.y1 > G.grid[1]) return false;
    for (int y = kr.y0; y < kr.y1; ++y)
        for (int x = kr.x0; x < kr.x1; ++x) {
            const uint32_t key = (uint32_t)(y * G.grid[0] + x);
            const uint32_t fb = key * (uint32_t)G.CT + (uint32_t)(G.CT - 1);
            if (fbits.full(key)) emit(fb, id | kUnsafe | kGeneral);
        }
    return true;
}

// Global fine cell (gx, gy) -> cell id (tile-major: tile * CT + fy * n + fx).
__device__ inline uint32_t cell_of(const Geom &G, int gx, int gy) {
    const int tx = gx / G.n, ty = gy / G.n;
    return (uint32_t)(ty * G.grid[0] + tx) * (uint32_t)G.CT + (uint32_t)((gy - ty * G.n) * G.n + (gx - tx * G.n));
}

// The cells a regular Gaussian's direct local tile visits emit (exactly those enumerate_fine
// skips for it), written as one global column range per global fine row: lrows[KR + dy][i] for
// row home_y + dy (|dy| <= reach), packed lo | hi << 16 (lo > hi: none).  Rows are walked in
// order, each row's tiles in turn, so a row's range is merged in registers and stored once.
// False if some row's cells are not one range (never for a convex cut; the Gaussian then stays
// on the sort path).
__device__ __forceinline__ bool local_rows(const Geom &G, const KeyRect &kr, const Cut &k, int home_y, int reach,
                                  int64_t P, int64_t i, uint32_t *__restrict__ lrows) {
    // Per Gaussian: the x tiles its cut can reach as a direct local visit (at most two: the cut is
    // narrower than a tile) with their cell ranges, and the slice constants.  These need not
    // match enumerate_fine bit for bit (it skips exactly these visits and emits all others); the
    // margins of the cut cover the rounding either way.
    const double BS = (double)kTile, slack = kCellSlack * G.fs;
    // (widened by a cell: every tile axis_setup can give a cell is among them -- which also
    // covers the rounding of the reciprocal multiply)
    const double wx = k.e[0] + slack + k.epsx[0] + G.fs, iBS = 1.0 / BS;
    const int ta = max(max(kr.x0, 0), (int)floor((k.md[0] - wx) * iBS));
    const int tb = min(min(kr.x1, G.grid[0]) - 1, (int)floor((k.md[0] + wx) * iBS));
    int xlo[2] = {1, 1}, xhi[2] = {0, 0};  // cell ranges of tiles ta, ta + 1 (empty: lo > hi)
    for (int t = 0; t < 2; ++t) {
        const int tx = ta + t;
        if (tx > tb) break;
        int ks[2] = {0, 0};
        // (every visit made here is local and the conic is not kUnsafe -- gather_reach --: the fast cut)
        if (axis_setup(G, k, 0, tx, ks[0], xlo[t], xhi[t]) && visit_local(G, k, ks) &&
            axis_fast(G, k, 0, tx, xlo[t], xhi[t]))
            continue;
        xlo[t] = 1; xhi[t] = 0;
    }
    if (tb > ta + 1) return false;  // (wider than two tiles: not for this path)
    // The row slices in fp32 (fp64 sqrt / division sequences were most of this kernel's issue
    // slots): coordinates relative to the tile origin, and margins that cover the fp32 rounding
    // -- the slice ends' error is at most ~sqrt(8 eps) of the cut's half-width where the sqrt
    // argument cancels (the ellipse's top and bottom), so tol = 2e-3 e0 + 1e-5 (1 + |x|) in
    // displacement units, a few thousandths of a cell.  Extra cells only add exact zeros.
    const float qc = (float)(G.qf * (1.0 + 1e-6));
    const float c0 = (float)k.c0, c1 = (float)k.c1, c2 = (float)k.c2;
    const float det = (float)(k.c0 * k.c2 - k.c1 * k.c1);
    // (e0: the cut's X0 half-width; k.ef[0] exceeds sqrt(qc c2 / det) by ~5e-7 relative, which
    // only widens the slices)
    const float e0 = (float)k.ef[0], ic0 = 1.0f / c0;
    const float yu0 = -c1 * e0 / c2, yl0 = c1 * e0 / c2, qcc0 = qc * c0;
    const float fs = (float)G.fs, ifsf = (float)G.ifs, slackf = (float)slack;
    const float e1 = (float)k.ef[1], eps1 = (float)k.epsx[1] + 1e-6f, eps0 = (float)k.epsx[0] + 1e-6f;
    const float tol0 = 2e-3f * e0 + 1e-5f;
    float A0[2], B0[2];  // per tile of the x range: the tile-relative mean +- the margins
    for (int t = 0; t < 2; ++t) {
        const float md0 = (float)(k.md[0] - (ta + t) * BS);
        A0[t] = md0 - slackf - eps0;
        B0[t] = md0 + slackf + eps0;
    }
    uint32_t written = 0u;  // bit KR + dy: row home_y + dy stored
    bool bad = false;       // (some row's cells are not one range, or a row is out of reach)
    const bool v0t = xlo[0] <= xhi[0], v1t = xlo[1] <= xhi[1];
    const float fn = (float)G.n;
    for (int ty = max(kr.y0, 0); ty < min(kr.y1, G.grid[1]); ++ty) {  // direct visits only
        int ks1, flo1, fhi1;
        if (!axis_setup(G, k, 1, ty, ks1, flo1, fhi1) || ks1 != 0 || !axis_fast(G, k, 1, ty, flo1, fhi1)) continue;
        const float md1 = (float)(k.md[1] - ty * BS);
        // (the row body without branches: its divergent continues / breaks were a third of
        // this kernel's instructions; partial stores of a Gaussian that ends up `bad` are never
        // read -- k_gather reads rows only of Gaussians with a reach)
        for (int fy = flo1; fy <= fhi1; ++fy) {
            const float ya = fmaxf(md1 - ((fy + 1) * fs + slackf) - eps1, -e1);
            const float yb = fminf(md1 - (fy * fs - slackf) + eps1, e1);
            const bool rowok = ya <= yb;
            const float yu = fminf(fmaxf(yu0, ya), yb), yl = fminf(fmaxf(yl0, ya), yb);
            // (v_sqrt_f32, ~1 ulp: far inside tol)
            const float xu = (-c1 * yu + __builtin_amdgcn_sqrtf(fmaxf(qcc0 - det * yu * yu, 0.0f))) * ic0;
            const float xl = (-c1 * yl - __builtin_amdgcn_sqrtf(fmaxf(qcc0 - det * yl * yl, 0.0f))) * ic0;
            const float tol = tol0 + 1e-5f * (fabsf(xu) + fabsf(xl));
            int a[2], b[2];
            bool v[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float fa = ceilf((A0[t] - (xu + tol)) * ifsf - 1.0f - 1e-4f);
                const float fb = floorf((B0[t] - (xl - tol)) * ifsf + 1e-4f);
                const int fxl = max(xlo[t], (int)fminf(fmaxf(fa, -1.0f), fn));
                const int fxh = min(xhi[t], (int)fmaxf(fminf(fb, fn), -1.0f));
                v[t] = (t == 0 ? v0t : v1t) && fxl <= fxh;
                a[t] = (ta + t) * G.n + fxl;
                b[t] = (ta + t) * G.n + fxh;
            }
            const int lo = v[0] ? a[0] : a[1], hi = v[1] ? b[1] : b[0];
            bad = bad || (rowok && v[0] && v[1] && a[1] != b[0] + 1);
            const int dy = ty * G.n + fy - home_y;
            const bool put = rowok && (v[0] || v[1]);
            const bool inr = dy >= -reach && dy <= reach;
            bad = bad || (put && !inr);
            if (put && inr) {
                lrows[(int64_t)(kGatherReach + dy) * P + i] = (uint32_t)lo | ((uint32_t)hi << 16);
                written |= 1u << (kGatherReach + dy);
            }
        }
    }
    if (bad) return false;
    uint32_t *rp = lrows + i;
#pragma unroll
    for (int q = 0; q < kGatherRows; ++q)
        if (q >= kGatherReach - reach && q <= kGatherReach + reach && !((written >> q) & 1u))
            rp[(int64_t)q * P] = 0x0000ffffu;
    return true;
}

__device__ inline void load_gauss(int D, const float *__restrict__ means,
                                  const float *__restrict__ conics, int64_t g, float *m, float *c) {
    const int S = D * (D + 1) / 2;
    m[0] = means[g * D];
    m[1] = D == 2 ? means[g * D + 1] : 0.0f;
    c[0] = conics[g * S];
    c[1] = D == 2 ? conics[g * S + 1] : 0.0f;
    c[2] = D == 2 ? conics[g * S + 2] : 0.0f;
}

// Bounding box of each cell's samples [min0 min1 max0 max1] (empty cells: unused).  One wave
// per cell, lanes striding over the cell's samples in the packed sorted rows (FsRows).
// (Both box kernels also set the fallback-cell bits fbg: tile t's bit when its fallback cell,
// cell t * CT + CT - 1, holds samples.)
__device__ __forceinline__ void set_fb_bit(int c, int CT, bool nonempty, uint32_t *__restrict__ fbg) {
    if (nonempty && c % CT == CT - 1) {
        const int t = c / CT;
        atomicOr(&fbg[t >> 5], 1u << (t & 31));
    }
}

__global__ __launch_bounds__(kBlock) void k_cell_box(int ncells, int D, int CT, const int32_t *__restrict__ sbeg,
                                                     const int32_t *__restrict__ send,
                                                     const float *__restrict__ rows,
                                                     float4 *__restrict__ box, uint32_t *__restrict__ fbg) {
    const int c = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & (kWave - 1);
    if (c >= ncells) return;
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    const int e = send[c];
    for (int j = sbeg[c] + lane; j < e; j += kWave) {
        const float *row = rows + (int64_t)(j >> 1) * (2 * D) + (j & 1);
        for (int d = 0; d < D; ++d) {
            const float v = row[2 * d];
            lo[d] = fminf(lo[d], v);
            hi[d] = fmaxf(hi[d], v);
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], off));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off));
        }
    if (D == 1) { lo[1] = hi[1] = 0.0f; }
    if (lane == 0) {
        box[c] = make_float4(lo[0], lo[1], hi[0], hi[1]);
        set_fb_bit(c, CT, send[c] > sbeg[c], fbg);
    }
}

// The Gaussians' records in internal order (k_gauss_prep's caller-order records gathered
// through perm): igm = mean, igc = (conic, radius), read coalesced by k_fine_count / k_fine_fill
// / k_geo_pack.  A kernel of its own: the random 32-byte gathers need many waves in flight
// (in k_fine_count they were a dependent round trip at its 4 waves per SIMD).
__global__ void k_gauss_permute(int P, const uint32_t *__restrict__ perm, const float4 *__restrict__ grec,
                                float2 *__restrict__ igm, float4 *__restrict__ igc, uint2 *__restrict__ irect) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int64_t g = perm[i];
    const float4 ga = grec[2 * g], gb = grec[2 * g + 1];
    igm[i] = make_float2(ga.x, ga.y);
    igc[i] = make_float4(ga.w, gb.x, gb.y, ga.z);
    irect[i] = make_uint2(__float_as_uint(gb.z), __float_as_uint(gb.w));
}

// Number of sort-path fine entries of each Gaussian (k_fine_fill writes them).  For the regular
// (gather-path) Gaussians also their reach and local row ranges (k_gather reads them as
// lrows[KR + dy][i]: coalesced over the contiguous id range of a home row), and the largest
// reach.  A regular Gaussian whose reference rect lies inside the grid counts its fallback
// entries here; every other one (irr: the per-Gaussian enumeration, long and uneven loops) is
// queued for k_fine_count_irr, so the waves here stay uniform.
// DGS_FC_PROF builds (tuning only): per-phase wave-cycle sums of k_fine_count (s_memtime at
// phase boundaries, lane 0 of each wave), read back with dgs_debug_fc_prof.
#ifndef DGS_FC_PROF
#define DGS_FC_PROF 0
#endif
#if DGS_FC_PROF
__device__ unsigned long long g_fc_prof[8];
#define FC_T(k) const uint64_t fc_t##k = __builtin_amdgcn_s_memtime()
#define FC_ADD(a, b, slot) if ((threadIdx.x & 63) == 0) atomicAdd(&g_fc_prof[slot], (unsigned long long)(fc_t##b - fc_t##a))
#else
#define FC_T(k)
#define FC_ADD(a, b, slot)
#endif

__global__ __launch_bounds__(kBlock) void k_fine_count(int P, Geom G, const float2 *__restrict__ igm,
                                                       const float4 *__restrict__ igc, const uint2 *__restrict__ irect,
                                                       const uint32_t *__restrict__ fbg,
                                                       uint64_t *__restrict__ counts, int8_t *__restrict__ greach,
                                                       uint32_t *__restrict__ lrows, int32_t *__restrict__ rmax,
                                                       uint32_t *__restrict__ irr, uint32_t *__restrict__ nirr,
                                                       int qcap, unsigned long long *__restrict__ nflag) {
    FC_T(0);
    const FbBits fbits = fb_load(fbg, G.T);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int reach = 0;
    bool queue = false;
    uint32_t nu = 0;  // kUnsafe entries (the regular Gaussians' fallback cells)
    FC_T(1);
    FC_ADD(0, 1, 0);
    if (i < P) {
        const float2 mm = igm[i];
        const float4 cc = igc[i];
        const float r = cc.w;
        uint64_t n = 0;
        const float m[2] = {mm.x, mm.y}, c[3] = {cc.x, cc.y, cc.z};
        FC_T(2);
        FC_ADD(1, 2, 1);
        if (r > 0.0f) {
            const Cut k = gauss_cut(G, m, c);
            const KeyRect kr = rect_get(irect[i], G.D, m, r, G);
            reach = gather_reach(G, m, r, c, k, kr);
            FC_T(3);
            FC_ADD(2, 3, 2);
            if (reach > 0) {
                const int home_y = (int)floor(((double)m[1] - (double)G.off[1]) * G.ifs);
                if (!local_rows(G, kr, k, home_y, reach, P, i, lrows)) reach = 0;
            }
            FC_T(4);
            FC_ADD(3, 4, 3);
            const auto count = [&](uint32_t, uint32_t v) {  // (fallback entries: kUnsafe)
                ++n;
                nu += (v & kUnsafe) ? 1u : 0u;
            };
            queue = !(reach > 0 && fallback_only(G, kr, fbits, (uint32_t)i, count));
            FC_T(5);
            FC_ADD(4, 5, 4);
        }
        counts[i] = n;
        greach[i] = (int8_t)reach;
    }
    // the wave's queued Gaussians take consecutive slots (one atomic per wave)
    const uint64_t qm = __ballot(queue);
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t qbase = 0;
    if (qm) {
        // (the queue in kShards parts, one counter each: in thin fields most waves queue)
        const int sh = shard_of_block();
        if (lane == 0) qbase = atomicAdd(&nirr[sh * kShard32], (uint32_t)__popcll(qm));
        qbase = __shfl(qbase, 0);
        if (queue) irr[(int64_t)sh * qcap + qbase + (uint32_t)__popcll(qm & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        reach = max(reach, __shfl_xor(reach, off));
        nu += __shfl_xor(nu, off);
    }
    // one sharded atomic per block for the largest reach, one per wave for rare unsafe counts
    __shared__ int bmax;
    if (threadIdx.x == 0) bmax = 0;
    __syncthreads();
    if (lane == 0 && reach > 0) atomicMax(&bmax, reach);
    __syncthreads();
    if (threadIdx.x == 0 && bmax > 0) atomicMax(&rmax[shard_of_block() * kShard32], bmax);
    if (lane == 0 && nu) atomicAdd(&nflag[shard_of_block() * kShard64], (unsigned long long)nu);
    FC_T(6);
    FC_ADD(0, 6, 5);
}

// The queued (irregular) Gaussians of k_fine_count: the per-Gaussian enumeration's count.
// Grid-strided over the device-side queue length.
__global__ __launch_bounds__(kBlock) void k_fine_count_irr(Geom G, const float2 *__restrict__ igm,
                                                           const float4 *__restrict__ igc, const int32_t *__restrict__ sbeg,
                                                           const int32_t *__restrict__ send, const float4 *__restrict__ box,
                                                           const uint32_t *__restrict__ fbg, const int8_t *__restrict__ greach,
                                                           const uint32_t *__restrict__ irr, const uint32_t *__restrict__ nirr,
                                                           int qcap, uint64_t *__restrict__ counts,
                                                           unsigned long long *__restrict__ nflag,
                                                           uint32_t *__restrict__ wq, uint32_t *__restrict__ nwq) {
    const FbBits fbits = fb_load(fbg, G.T);
    uint32_t nu = 0, nt = 0;  // kUnsafe / kThin entries (k_fine_fill emits the same ones): read back at the sync
    // (the queue's parts, as one index range over their concatenation)
    uint32_t pre[kShards + 1];
    pre[0] = 0;
#pragma unroll
    for (int sh = 0; sh < kShards; ++sh) pre[sh + 1] = pre[sh] + sload(&nirr[sh * kShard32]);
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < pre[kShards]; q += gridDim.x * blockDim.x) {
        int sh = 0;
#pragma unroll
        for (int k = 1; k < kShards; ++k) sh += q >= pre[k] ? 1 : 0;
        const uint32_t i = irr[(int64_t)sh * qcap + (q - pre[sh])];
        const float2 mm = igm[i];
        const float4 cc = igc[i];
        const float m[2] = {mm.x, mm.y}, c[3] = {cc.x, cc.y, cc.z};
        const Cut k = gauss_cut(G, m, c);
        // (k_wide counts the unculled ones: one queue append per wave, consecutive slots -- a field
        // of non-positive-definite conics must not serialise on one counter)
        const bool wide = wide_gauss(k);
        const uint64_t wm = __ballot(wide);
        if (wm) {
            const int lane = threadIdx.x & (kWave - 1), lead = __ffsll((unsigned long long)wm) - 1;
            uint32_t wbase = 0;
            if (lane == lead) wbase = atomicAdd(nwq, (uint32_t)__popcll(wm));
            wbase = __shfl(wbase, lead);
            if (wide) wq[wbase + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull))] = i;
        }
        if (wide) continue;
        uint64_t n = 0;
        const auto count = [&](uint32_t, uint32_t v) {
            ++n;
            nu += (v & kUnsafe) ? 1u : 0u;
            nt += (v & kThin) ? 1u : 0u;
        };
        enumerate_fine(G, m, cc.w, c, k, greach[i] > 0, sbeg, send, box, fbits, i, count);
        counts[i] = n;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        nu += __shfl_xor(nu, off);
        nt += __shfl_xor(nt, off);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {  // (sharded: see kShards)
        if (nu) atomicAdd(&nflag[shard_of_block() * kShard64], (unsigned long long)nu);
        if (nt) atomicAdd(&nflag[shard_of_block() * kShard64 + 1], (unsigned long long)nt);
    }
}

// (cell, class) sort key of an entry: flag-free, flagged, then the thin (kThin) ones last in a
// cell -- the forward's main and thin passes then meet few mixed groups; key >> 1 = (cell, flagged)
__device__ __forceinline__ uint32_t entry_key(uint32_t cell, uint32_t val) {
    return (cell << 2) | ((val & kSlow) ? 2u : 0u) | ((val & kThin) ? 1u : 0u);
}

// Unculled Gaussians (not positive definite, past kRho2Max, or a cut half-width >= 0.5) enter
// every non-empty fine cell of every tile of their rect: ~1500 entries each.  One thread per
// Gaussian (enumerate_fine) made them a serial tail -- 107 such Gaussians of the axis-ratio-25
// field held k_fine_count_irr and k_fine_fill at 1.7 and 2.4 ms.  Here one wave per Gaussian,
// lanes over a tile's cells in index order, emits the same entries in the same order
// (enumerate_fine with cull = false: every tile of the rect, cells 0 .. n^D - 1 that hold
// samples, classified by their sample box, then the tile's fallback cell when it holds samples).
// k_fine_count_irr queues them (wq); !FILL counts (counts[i], the kUnsafe / kThin totals), FILL
// writes them from offs[i] on.

template <bool FILL, typename KT>
__global__ __launch_bounds__(kBlock) void k_wide(Geom G, const float2 *__restrict__ igm, const float4 *__restrict__ igc,
                                                 const int32_t *__restrict__ sbeg, const int32_t *__restrict__ send,
                                                 const float4 *__restrict__ box, const uint32_t *__restrict__ fbg,
                                                 const uint32_t *__restrict__ wq, const uint32_t *__restrict__ nwq,
                                                 uint64_t *__restrict__ counts, const uint64_t *__restrict__ offs,
                                                 KT *__restrict__ ekeys, uint32_t *__restrict__ evals, uint64_t cap,
                                                 unsigned long long *__restrict__ nflag, int32_t *__restrict__ counters) {
    const FbBits fbits = fb_load(fbg, G.T);
    const int D = G.D, lane = threadIdx.x & (kWave - 1);
    const uint64_t below = (1ull << lane) - 1ull;
    const int nc = D == 2 ? G.n * G.n : G.n;
    const uint32_t nq = sload(nwq);
    uint32_t nu = 0, nt = 0;
    for (uint32_t q = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); q < nq; q += gridDim.x * kWavesPerBlock) {
        const uint32_t i = __builtin_amdgcn_readfirstlane(wq[q]);
        const float2 mm = igm[i];
        const float4 cc = igc[i];
        const float m[2] = {mm.x, mm.y}, con[3] = {cc.x, cc.y, cc.z};
        const KeyRect kr = ref_key_rect(D, m, cc.w, G.grid, G.off);
        const uint32_t uflag = conic_unsafe(D, con[0], con[1], con[2]) ? kUnsafe : 0u;
        uint64_t o = FILL ? offs[i] : 0;
        for (int y = kr.y0; y < kr.y1; ++y)
            for (int x = kr.x0; x < kr.x1; ++x) {
                const uint32_t key = key_of(D, x, y, G.grid);
                if (key >= (uint32_t)G.T) continue;
                const uint32_t base = key * (uint32_t)G.CT;
                for (int j0 = 0; j0 < nc; j0 += kWave) {
                    const int j = j0 + lane;
                    bool hit = false;
                    uint32_t val = 0;
                    if (j < nc) {
                        const uint32_t cell = base + (uint32_t)j;
                        if (send[cell] > sbeg[cell]) {  // (enumerate_fine's classification, !local)
                            const float4 bx = box[cell];
                            const double blo[2] = {bx.x, bx.y}, bhi[2] = {bx.z, bx.w};
                            bool inside = true, constant = true;
#pragma unroll
                            for (int d = 0; d < 2; ++d) {
                                if (d >= D) break;
                                const double eps =
                                    1e-6 * (1.0 + fabs((double)m[d]) + fmax(fabs(blo[d]), fabs(bhi[d])));
                                const double wa = (double)m[d] - bhi[d] - eps, wb = (double)m[d] - blo[d] + eps;
                                inside = inside && wa >= -1.0 && wb <= 1.0;
                                constant = constant && wrap_shift(wa) == wrap_shift(wb);
                            }
                            hit = true;
                            val = i | uflag | (inside ? 0u : (constant ? kGeneral : kGeneral | kUnsafe));
                        }
                    }
                    const uint64_t hm = __ballot(hit);
                    if (hit) {
                        nu += (val & kUnsafe) ? 1u : 0u;
                        nt += (val & kThin) ? 1u : 0u;
                        if (FILL) {
                            const uint64_t at = o + (uint64_t)__popcll(hm & below);
                            if (at < cap) {
                                ekeys[at] = (KT)entry_key(base + (uint32_t)j, val);
                                evals[at] = val;
                            }
                        }
                    }
                    o += (uint64_t)__popcll(hm);
                }
                if (fbits.full(key)) {  // whole tile: general path
                    const uint32_t cell = base + (uint32_t)(G.CT - 1), val = i | kUnsafe | kGeneral;
                    if (lane == 0) {
                        ++nu;
                        if (FILL && o < cap) {
                            ekeys[o] = (KT)entry_key(cell, val);
                            evals[o] = val;
                        }
                    }
                    ++o;
                }
            }
        if (!FILL && lane == 0) counts[i] = o;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        nu += __shfl_xor(nu, off);
        nt += __shfl_xor(nt, off);
    }
    if (lane == 0) {
        if (FILL) {
            if (nu) atomicAdd(reinterpret_cast<uint32_t *>(&counters[kNumUnsafe]), nu);
        } else {  // (k_fine_count_irr's totals, read back at the sync)
            if (nu) atomicAdd(&nflag[shard_of_block() * kShard64], (unsigned long long)nu);
            if (nt) atomicAdd(&nflag[shard_of_block() * kShard64 + 1], (unsigned long long)nt);
        }
    }
}

// The block's Gaussians own one contiguous output range (offs is an exclusive scan in i
// order); it is staged in LDS and written out coalesced when it fits (per-lane runs of ~15
// entries at 64 different addresses per store were most of this kernel's time).  A block with
// an unculled (k_wide) Gaussian writes directly: k_wide fills that Gaussian's part of the range.
#ifndef DGS_FILL_CAP
#define DGS_FILL_CAP 3072
#endif
constexpr int kFillBlock = 128, kFillCap = DGS_FILL_CAP;

// KT: the entry key type -- uint16_t when every (cell, flag) key fits 16 bits (the radix sort
// then moves 6 instead of 8 bytes per entry and pass).
template <typename KT>
__global__ __launch_bounds__(kFillBlock) void k_fine_fill(
    int P, Geom G, const float2 *__restrict__ igm, const float4 *__restrict__ igc, const int32_t *__restrict__ sbeg,
    const int32_t *__restrict__ send, const float4 *__restrict__ box, const uint64_t *__restrict__ offs,
    const uint64_t *__restrict__ cnts, const int8_t *__restrict__ greach, const uint32_t *__restrict__ fbg,
    const uint2 *__restrict__ irect, KT *__restrict__ ekeys, uint32_t *__restrict__ evals,
    int32_t *__restrict__ counters, uint64_t cap) {  // cap: the arrays' capacity (capturable binning)
    __shared__ uint32_t skey[kFillCap], sval[kFillCap];
    const FbBits fbits = fb_load(fbg, G.T);
    const int64_t i0 = (int64_t)blockIdx.x * kFillBlock;
    const int64_t i = i0 + threadIdx.x;
    const int64_t ilast = min((int64_t)P, i0 + kFillBlock) - 1;
    const uint64_t base = offs[i0], end = offs[ilast] + cnts[ilast];
    bool mine = i < P && cnts[i] > 0;
    float m[2] = {0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f}, r = 0.0f;
    Cut k;
    if (mine) {
        const float2 mm = igm[i];
        const float4 cc = igc[i];
        m[0] = mm.x, m[1] = mm.y, c[0] = cc.x, c[1] = cc.y, c[2] = cc.z, r = cc.w;
        k = gauss_cut(G, m, c);
    }
    const bool wide = mine && wide_gauss(k);
    const bool stage = __syncthreads_or(wide) == 0 && end - base <= (uint64_t)kFillCap;
    mine = mine && !wide;
    uint32_t nunsafe = 0;
    if (mine) {
        const bool skip = greach[i] > 0;  // (k_fine_count's decision)
        uint64_t o = offs[i];
        const auto put = [&](uint32_t cell, uint32_t val) {
            const uint32_t key = entry_key(cell, val);
            if (stage) {
                skey[o - base] = key;
                sval[o - base] = val;
            } else if (o < cap) {
                ekeys[o] = (KT)key;
                evals[o] = val;
            }
            nunsafe += (val & kUnsafe) ? 1u : 0u;
            ++o;
        };
        if (!(skip && fallback_only(G, rect_get(irect[i], 2, m, r, G), fbits, (uint32_t)i, put)))
            enumerate_fine(G, m, r, c, k, skip, sbeg, send, box, fbits, (uint32_t)i, put);
    }
    for (int off = kWave / 2; off > 0; off >>= 1) nunsafe += __shfl_xor(nunsafe, off);
    if ((threadIdx.x & (kWave - 1)) == 0 && nunsafe)  // (one add per wave that has any)
        atomicAdd(reinterpret_cast<uint32_t *>(&counters[kNumUnsafe]), nunsafe);
    if (stage) {
        __syncthreads();
        const int n = (int)(end - base);
        for (int k = threadIdx.x; k < n; k += kFillBlock) {
            if (base + k >= cap) break;
            ekeys[base + k] = (KT)skey[k];
            evals[base + k] = sval[k];
        }
    }
}

// hstart[h] = first internal id whose home cell is >= h (lower bound in the sorted home keys),
// h in [0, HK]; home cell h's Gaussians are ids [hstart[h], hstart[h + 1]).
__global__ void k_home_start(int P, int HK, const uint32_t *__restrict__ home_sorted, uint32_t *__restrict__ hstart) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h > HK) return;
    int lo = 0, hi = P;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (home_sorted[mid] < (uint32_t)h) lo = mid + 1;
        else hi = mid;
    }
    hstart[h] = (uint32_t)lo;
}

// Per-cell gather of the regular Gaussians' local entries (D = 2): one wave per (strip of
// kStripW cells of a global fine row gy, home row offset dy).  Its candidates are the Gaussians
// homed in row gy - dy within the largest reach R of the strip -- one contiguous id range, read
// in ascending id with their precomputed column ranges for row gy (lrows).  !FILL: count per
// (cell, dy) and in total (eg); FILL: write them, home rows in ascending order (dy descending)
// after each other, so every cell's gathered entries are in ascending id (the backward's atomics
// need that order) with no sort.
constexpr int kStripW = 32;
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_gather(Geom G, int P, const int8_t *__restrict__ greach,
                                                   const uint32_t *__restrict__ lrows,
                                                   const uint32_t *__restrict__ hstart,
                                                   const int32_t *__restrict__ rmax, uint32_t *__restrict__ cnt2,
                                                   unsigned long long *__restrict__ eg,
                                                   const int32_t *__restrict__ gbeg, uint32_t *__restrict__ entries,
                                                   uint32_t ecap = 0xffffffffu) {
    const int home_w = G.grid[0] * G.n, home_h = G.grid[1] * G.n;
    const int spr = (home_w + kStripW - 1) / kStripW;
    const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6));
    const int strip = wid / kGatherRows, q = wid - strip * kGatherRows, dy = q - kGatherReach;
    if (strip >= home_h * spr) return;
    int R = 0;
#pragma unroll
    for (int q2 = 0; q2 < kShards; ++q2) R = max(R, sload(&rmax[q2 * kShard32]));
    const int gy = strip / spr, gx0 = (strip - gy * spr) * kStripW, nw = min(kStripW, home_w - gx0);
    const int hy = gy - dy;
    if (dy < -R || dy > R || hy < 0 || hy >= home_h) return;  // (cnt2 stays 0 there)
    const int lane = threadIdx.x & (kWave - 1);
    // lane j < nw keeps cell gx0 + j's cursor (FILL: its next slot; else its count)
    uint32_t cur = 0;
    if (FILL && lane < nw) {
        const uint32_t c = cell_of(G, gx0 + lane, gy);
        cur = (uint32_t)gbeg[c];
        for (int q2 = q + 1; q2 < kGatherRows; ++q2) cur += cnt2[(int64_t)c * kGatherRows + q2];  // lower home rows
    }
    const int clo = max(gx0 - R, 0), chi = min(gx0 + nw - 1 + R, home_w - 1);
    const uint32_t ib = sload(&hstart[hy * home_w + clo]), ie = sload(&hstart[hy * home_w + chi + 1]);
    const int ady = dy < 0 ? -dy : dy;
    const uint32_t *__restrict__ lq = lrows + (int64_t)q * P;
    // the next chunk's reach and row range are loaded while a chunk is processed (both at once:
    // a row range past the Gaussian's reach is never used, only read)
    int rch_n = 0;
    uint32_t rr_n = 0u;
    if (ib + lane < ie) { rch_n = greach[ib + lane]; rr_n = lq[ib + lane]; }
    for (uint32_t i0 = ib; i0 < ie; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const int rch = rch_n;
        const uint32_t rr = rr_n;
        if (i + kWave < ie) { rch_n = greach[i + kWave]; rr_n = lq[i + kWave]; }
        uint32_t mask = 0u;
        if (i < ie && rch >= ady && rch > 0) {
            const int a = max((int)(rr & 0xffffu), gx0) - gx0, b = min((int)(rr >> 16), gx0 + nw - 1) - gx0;
            if (a <= b) mask = (b >= 31 ? 0xffffffffu : ((2u << b) - 1u)) & ~((1u << a) - 1u);
        }
        uint32_t any = mask;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) any |= __shfl_xor(any, off);
        any = __builtin_amdgcn_readfirstlane(any);
        while (any) {
            const int j = __builtin_ctz(any);
            any &= any - 1u;
            const bool hit = (mask >> j) & 1u;
            const uint64_t bal = __ballot(hit);
            if (FILL) {
                const uint32_t base = __builtin_amdgcn_readlane(cur, j);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                if (hit && base + rank < ecap) entries[base + rank] = i;
            }
            if (lane == j) cur += (uint32_t)__popcll(bal);
        }
    }
    if (!FILL) {
        if (lane < nw) cnt2[(int64_t)cell_of(G, gx0 + lane, gy) * kGatherRows + q] = cur;
        unsigned long long t = lane < nw ? cur : 0u;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0 && t) atomicAdd(&eg[shard_of_block() * kShard64], t);  // (sharded: see kShards)
    }
}

// The sorted path's half-cells copied behind each cell's gathered entries (one wave per cell).
// The sorted path's entries copied behind each cell's gathered ones, one thread per sorted
// position r: its key gives the cell and the class (key >> 1 = (cell, flagged)), hb the class's
// first sorted position.  sq: the sort's values, the entries' Gaussian-major positions q
// (k_fine_fill's order); the entry itself is evals[q], and q is kept as the list position's
// backward slot (esum_q).
template <typename KT>
__global__ void k_copy_sorted(int64_t Es, const KT *__restrict__ keys, const uint32_t *__restrict__ sq,
                              const uint32_t *__restrict__ evals, const int32_t *__restrict__ hb,
                              const int32_t *__restrict__ gbeg, const int32_t *__restrict__ gmid,
                              const uint32_t *__restrict__ gcnt, uint32_t *__restrict__ entries,
                              uint32_t *__restrict__ esum_q, const int64_t *__restrict__ Esdev, int64_t Ecap) {
    if (Esdev) Es = min(Es, max(sload(Esdev), (int64_t)0));  // (capturable binning: the device count)
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= Es) return;
    const uint32_t key = (uint32_t)keys[r], c = key >> 2;
    const bool fl = (key >> 1) & 1u;
    const int64_t p = fl ? (int64_t)gmid[c] + (r - hb[2 * c + 1]) : (int64_t)gbeg[c] + gcnt[c] + (r - hb[2 * c]);
    if (p >= Ecap) return;
    const uint32_t q = sq[r];
    entries[p] = evals[q];
    esum_q[p] = q;
}

// D = 2: the bounding boxes of a cell's four sub-cells and of the cell (their union), one wave
// per cell.  Empty sub-cells get an empty box (+inf lo, -inf hi).
__global__ __launch_bounds__(kBlock) void k_sub_box(int ncells, int CT, const int32_t *__restrict__ ssbeg,
                                                    const int32_t *__restrict__ ssend,
                                                    const float *__restrict__ rows, float4 *__restrict__ sbox,
                                                    float4 *__restrict__ box, uint32_t *__restrict__ fbg) {
    const int c = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & (kWave - 1);
    if (c >= ncells) return;
    float clo[2] = {INFINITY, INFINITY}, chi[2] = {-INFINITY, -INFINITY};
    for (int k = 0; k < kSubPerCell; ++k) {
        const int sc = c * kSubPerCell + k;
        float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
        const int e = ssend[sc];
        for (int j = ssbeg[sc] + lane; j < e; j += kWave) {
            const float *row = rows + (int64_t)(j >> 1) * 4 + (j & 1);
            for (int d = 0; d < 2; ++d) {
                const float v = row[2 * d];
                lo[d] = fminf(lo[d], v);
                hi[d] = fmaxf(hi[d], v);
            }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                lo[d] = fminf(lo[d], __shfl_xor(lo[d], off));
                hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off));
            }
        if (lane == 0) sbox[sc] = make_float4(lo[0], lo[1], hi[0], hi[1]);
        for (int d = 0; d < 2; ++d) { clo[d] = fminf(clo[d], lo[d]); chi[d] = fmaxf(chi[d], hi[d]); }
    }
    if (lane == 0) {
        box[c] = make_float4(clo[0], clo[1], chi[0], chi[1]);
        set_fb_bit(c, CT, clo[0] <= chi[0], fbg);
    }
}

#ifndef DGS_SUBL_DEPTH
#define DGS_SUBL_DEPTH 2  // k_sub_lists: Gaussian-row groups in flight ahead of the tested one (1: 24 us slower at the headline)
#endif
#ifndef DGS_SUB_SLICE
#define DGS_SUB_SLICE 1  // k_sub_lists: per-sub-row slices instead of per-sub-box minimisations
#endif
// Does the box [xa, xb] x [ya, yb] of displacements contain an X with X^T A X <= qcut?  fp32
// with the reciprocals of c0 / c2 given (the sub-cell test runs once per entry and sub-cell).
// Rounding moves the computed minimum by ~1e-6 relative; the callers' qcut has a 1e-4 margin and
// the live pairs end at 207.9 (expf underflow; 175.51 on the fast paths, cut 176), so a live pair is never culled.
__device__ inline bool box_hits_ellipse_f(float xa, float xb, float ya, float yb, float c0, float c1, float c2,
                                          float ic0, float ic2, float qcut) {
    if (xa <= 0.0f && xb >= 0.0f && ya <= 0.0f && yb >= 0.0f) return true;
    float best = INFINITY;
    const float xs[2] = {xa, xb}, ys[2] = {ya, yb};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float x = xs[k];
        const float y = fminf(fmaxf(-c1 * x * ic2, ya), yb);
        best = fminf(best, c0 * x * x + 2.0f * c1 * x * y + c2 * y * y);
        const float yy = ys[k];
        const float xx = fminf(fmaxf(-c1 * yy * ic0, xa), xb);
        best = fminf(best, c0 * xx * xx + 2.0f * c1 * xx * yy + c2 * yy * yy);
    }
    return best <= qcut;
}

// The sub-cells of one cell a cell-list entry's cut X^T A X <= kQCut (flag-free: G.qf) meets (bit k = sub-cell k),
// tested with the displacement the forward uses: X = m - s, minus the entry's constant wrap
// shift for kGeneral entries (wrap_shift_f of the mean minus the cell-box centre, exactly as
// k_forward_t forms it).  kUnsafe entries get none (the forward's tail pass adds them per cell).
// (the entry's Gaussian, loaded a group ahead by k_sub_lists; zeros for kUnsafe entries)
__device__ __forceinline__ void sub_row(uint32_t ent, const float2 *__restrict__ gmean, const float4 *__restrict__ gcon,
                                        float2 &mm, float4 &cc) {
    mm = make_float2(0.0f, 0.0f);
    cc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(ent & kUnsafe)) {
        const uint32_t id = ent & kIdMask;
        mm = gmean[id];
        cc = gcon[id];
    }
}

__device__ __forceinline__ uint32_t sub_mask(uint32_t ent, const float2 &mm, const float4 &cc, const float4 &bx,
                                             const float *ctr, const float4 *sb, float qcf) {
    if (ent & kUnsafe) return 0u;
    // A flag-free entry (the k = 0 image, a conic that is not kUnsafe) is evaluated by the fast
    // paths alone: the fast cut qcf = G.qf (1 + 1e-4) (dgs_internal.h, kQCutFast).  A kGeneral
    // entry is a torus-shifted image: the reference cut.
    const float qc = (ent & kGeneral) ? (float)(kQCut * (1.0 + 1e-4)) : qcf;
    float sh[2] = {0.0f, 0.0f};
    if (ent & kGeneral) {
        sh[0] = wrap_shift_f(mm.x - ctr[0]);
        sh[1] = wrap_shift_f(mm.y - ctr[1]);
    }
    const float m0 = mm.x - sh[0], m1 = mm.y - sh[1];  // (exact: Sterbenz / even shifts)
    // (approximate reciprocals and square roots -- v_rcp_f32 / v_sqrt_f32, ~1 ulp: they place
    // the slice ends, whose error the 1e-4 margin on the cut and tol cover; rounding margins from
    // the cell box, which holds every sub-cell box)
    const float ic0 = __builtin_amdgcn_rcpf(cc.x), ic2 = __builtin_amdgcn_rcpf(cc.z);
    const float e0 = 1e-6f * (1.0f + fabsf(mm.x) + fmaxf(fabsf(bx.x), fabsf(bx.z)));
    const float e1 = 1e-6f * (1.0f + fabsf(mm.y) + fmaxf(fabsf(bx.y), fabsf(bx.w)));
    uint32_t mask = 0u;
#if DGS_SUB_SLICE
    // Per sub-row (the union of its two sub-boxes' sample y ranges) the ellipse's slice is one
    // X0 interval [xl, xu] (row_slice's construction in fp32); a sub-box is hit when its X0
    // range meets it.  Two slices per entry instead of four box minimisations.  The union band
    // and the tolerances only widen the lists (the cut itself sits outside the last live pair:
    // kQCut by 1 %, kQCutFast by 0.3 % -- 175.51 against 176, dgs_internal.h).
    const float c0 = cc.x, c1 = cc.y, c2 = cc.z;
    const float det = c0 * c2 - c1 * c1;
    const float ex0 = __builtin_amdgcn_sqrtf(qc * c2 * __builtin_amdgcn_rcpf(det));
    const float ex1 = __builtin_amdgcn_sqrtf(qc * c0 * __builtin_amdgcn_rcpf(det));
    const float yu0 = -c1 * ex0 * ic2;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float blo = fminf(sb[2 * r].y, sb[2 * r + 1].y), bhi = fmaxf(sb[2 * r].w, sb[2 * r + 1].w);
        const float ya = fmaxf(m1 - bhi - e1, -ex1), yb = fminf(m1 - blo + e1, ex1);
        if (!(ya <= yb)) continue;  // (also: both sub-boxes of the row empty)
        const float yu = fminf(fmaxf(yu0, ya), yb), yl = fminf(fmaxf(-yu0, ya), yb);
        const float xu = (-c1 * yu + __builtin_amdgcn_sqrtf(fmaxf(qc * c0 - det * yu * yu, 0.0f))) * ic0;
        const float xl = (-c1 * yl - __builtin_amdgcn_sqrtf(fmaxf(qc * c0 - det * yl * yl, 0.0f))) * ic0;
        const float tol = 1e-5f * (1.0f + fabsf(xu) + fabsf(xl));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 q = sb[2 * r + h];
            if (q.x <= q.z && m0 - q.z - e0 <= xu + tol && m0 - q.x + e0 >= xl - tol) mask |= 1u << (2 * r + h);
        }
    }
#else
    for (int k = 0; k < kSubPerCell; ++k) {
        const float4 q = sb[k];
        if (!(q.x <= q.z)) continue;  // empty sub-cell
        if (box_hits_ellipse_f(m0 - q.z - e0, m0 - q.x + e0, m1 - q.w - e1, m1 - q.y + e1, cc.x, cc.y, cc.z, ic0,
                               ic2, qc))
            mask |= 1u << k;
    }
#endif
    return mask;
}

// Sub lists (D = 2), one pass, one wave per cell: for every entry of the cell list, the
// sub-cells whose sample box its cut meets (sub_mask).  Sub list k of the cell has the region
// [4 gbeg + k n, + n) of sub_ent (n = the cell list's length: an entry is in at most every sub
// list of its cell); it is written in cell-list order, so [lbeg, lmid) holds the flag-free
// entries, [lmid, lend) the flagged ones (lthin = lend: no kThin entries since round 6).  The next group's Gaussian rows and the one
// after's entries are loaded while a group is tested (one stage: waves parked on the row
// gathers half their cycles, PMC SQ_WAIT_ANY).  (A block-per-cell form -- masks
// of the whole list in parallel into LDS, then one compacting wave per sub list -- was slower:
// 235 against 182 us at the headline, the same math plus the LDS round trip.)
struct SubListArgs {
    int ncells, CT;
    const int32_t *gbeg, *gmid, *gend;
    const uint32_t *entries;
    const float2 *gmean;
    const float4 *gcon, *box, *sbox;
    int32_t *lbeg, *lmid, *lend, *lthin;
    uint32_t *sub_ent;
    float qcf;  // the flag-free entries' cut, G.qf (1 + 1e-4)
};

__device__ __forceinline__ void sub_lists_wave(const SubListArgs &A, int c, int lane) {
    const int32_t *__restrict__ gbeg = A.gbeg, *__restrict__ gmid = A.gmid, *__restrict__ gend = A.gend;
    const uint32_t *__restrict__ entries = A.entries;
    const float2 *__restrict__ gmean = A.gmean;
    const float4 *__restrict__ gcon = A.gcon, *__restrict__ box = A.box, *__restrict__ sbox = A.sbox;
    int32_t *__restrict__ lbeg = A.lbeg, *__restrict__ lmid = A.lmid, *__restrict__ lend = A.lend;
    int32_t *__restrict__ lthin = A.lthin;
    uint32_t *__restrict__ sub_ent = A.sub_ent;
    const int CT = A.CT;
    const int b = gbeg[c], m_ = gmid[c], e = gend[c], n = e - b;
    uint32_t nff[kSubPerCell] = {0, 0, 0, 0}, nfl[kSubPerCell] = {0, 0, 0, 0};
    const int64_t base = (int64_t)kSubPerCell * b;
    if (b < e && (c % CT) != CT - 1) {  // (the fallback cell: every entry is kUnsafe)
        const float4 bx = box[c];
        const float ctr[2] = {0.5f * (bx.x + bx.z), 0.5f * (bx.y + bx.w)};  // = cell_center
        float4 sb[kSubPerCell];
#pragma unroll
        for (int k = 0; k < kSubPerCell; ++k) sb[k] = sbox[c * kSubPerCell + k];
        // two-stage pipeline: group g + 1's Gaussians and group g + 2's entries are in flight
        // while group g is tested
        uint32_t ent_c = b + lane < e ? entries[b + lane] : kUnsafe;
        uint32_t ent_n = b + kWave + lane < e ? entries[b + kWave + lane] : kUnsafe;
        float2 mm_c;
        float4 cc_c;
        sub_row(ent_c, gmean, gcon, mm_c, cc_c);
#if DGS_SUBL_DEPTH > 1
        // (three stages: group g + 1's and g + 2's Gaussians, g + 3's entries)
        float2 mm_n;
        float4 cc_n;
        sub_row(ent_n, gmean, gcon, mm_n, cc_n);
        uint32_t ent_nn = b + 2 * kWave + lane < e ? entries[b + 2 * kWave + lane] : kUnsafe;
#endif
        for (int j0 = b; j0 < e; j0 += kWave) {
            const int j = j0 + lane;
            const uint32_t ent = ent_c;
            const float2 mm = mm_c;
            const float4 cc = cc_c;
#if DGS_SUBL_DEPTH > 1
            ent_c = ent_n;
            mm_c = mm_n;
            cc_c = cc_n;
            ent_n = ent_nn;
            sub_row(ent_n, gmean, gcon, mm_n, cc_n);
            ent_nn = j + 3 * kWave < e ? entries[j + 3 * kWave] : kUnsafe;
#else
            ent_c = ent_n;
            sub_row(ent_c, gmean, gcon, mm_c, cc_c);
            ent_n = j + 2 * kWave < e ? entries[j + 2 * kWave] : kUnsafe;
#endif
            const uint32_t mask = j < e ? sub_mask(ent, mm, cc, bx, ctr, sb, A.qcf) : 0u;
            const bool ff = j < m_;
#pragma unroll
            for (int k = 0; k < kSubPerCell; ++k) {
                const bool hit = (mask >> k) & 1u;
                const uint64_t bf = __ballot(hit && ff), bl = __ballot(hit && !ff);
                if (hit) {
                    const uint32_t below = (uint32_t)__popcll((ff ? bf : bl) & ((1ull << lane) - 1ull));
                    // flag-free entries precede the flagged ones in the cell list, so once a group
                    // holds a flagged entry the flag-free count is final -- this group's own
                    // flag-free hits included: the region fills [flag-free | flagged] in order
                    const uint32_t nffk = nff[k] + (uint32_t)__popcll(bf);
                    const int64_t o = base + (int64_t)k * n + (ff ? nff[k] : nffk + nfl[k]) + below;
                    sub_ent[o] = ent;
                }
                nff[k] += (uint32_t)__popcll(bf);
                nfl[k] += (uint32_t)__popcll(bl);
            }
        }
    }
    if (lane == 0)
        for (int k = 0; k < kSubPerCell; ++k) {
            const int a = (int)(base + (int64_t)k * n);
            lbeg[c * kSubPerCell + k] = a;
            lmid[c * kSubPerCell + k] = a + (int)nff[k];
            lend[c * kSubPerCell + k] = a + (int)(nff[k] + nfl[k]);
            lthin[c * kSubPerCell + k] = a + (int)(nff[k] + nfl[k]);  // (no kThin entries since round 6: = lend)
        }
}

__global__ __launch_bounds__(kBlock) void k_sub_lists(SubListArgs A) {
    const int c = block_unit_index() * (kBlock / kWave) + (threadIdx.x >> 6);  // (XCD remap: neighbouring cells share Gaussians)
    if (c >= A.ncells) return;
    sub_lists_wave(A, c, threadIdx.x & (kWave - 1));
}

// (The per-cell list sizes and layout, the forward / backward work units and the forward sub
// units are each one fused_scan launch in preprocess_body: counts -> scan -> outputs.)

// duplicateWithKeys (sampler_impl.cu:54-129) without the 64-bit key: every Gaussian writes
// its tiles, in the reference's order, at its scan offset (caller id order); a stable sort by
// tile then yields the reference's point_list (ascending id per tile) -- the pair set of the
// call-time path (dgs_reference.hip).
// Run lazily (ensure_ref_lists) over the internal ids: the binned means (gmean), radius and
// tile-list offset (rref) of caller id g = perm[i].
// (Writes stay below R, the list size the scratch was sized for: a capturable binning clamps its
// header's R to capacity_R while the offsets keep the true counts.)
__global__ void k_ref_keys(int P, int64_t R, Geom G, const float2 *__restrict__ gmean, const int32_t *__restrict__ perm,
                           const uint32_t *__restrict__ rref, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float r = __uint_as_float(rref[P + i]);  // (radius, internal order)
    if (!(r > 0.0f)) return;
    const int64_t g = perm[i];
    const float2 mm = gmean[i];
    const float m[2] = {mm.x, mm.y};
    const KeyRect kr = ref_key_rect(G.D, m, r, G.grid, G.off);
    uint64_t o = rref[g];  // (tile-list offset, caller order)
    for (int y = kr.y0; y < kr.y1; ++y)
        for (int x = kr.x0; x < kr.x1 && (int64_t)o < R; ++x) {
            keys[o] = key_of(G.D, x, y, G.grid);
            vals[o] = (uint32_t)g;
            ++o;
        }
}

// Reference-layout ranges (identifyTileRanges semantics: empty tiles stay (0, 0)) for the
// Gaussian and the sample lists, and the call-time path's per-tile tables (RefTab): list
// starts and unit prefix counts.  One block; each thread scans a contiguous run of tiles.
__device__ __forceinline__ void ref_tables_block(int T, const uint32_t *__restrict__ gcnt,
                                                 const uint32_t *__restrict__ scnt,
                                                 uint2 *__restrict__ granges, uint2 *__restrict__ sranges,
                                                 uint32_t *__restrict__ rtab) {
    __shared__ uint4 part[kBlock];
    const int nt = blockDim.x, t = threadIdx.x;
    const int per = (T + nt - 1) / nt, a = min(T, t * per), b = min(T, a + per);
    uint4 sum = make_uint4(0u, 0u, 0u, 0u);
    // gcnt / scnt: kShards copies of T + 1 counts
    const auto tcount = [&](const uint32_t *cnt, int k) {
        uint32_t v = 0;
        for (int q = 0; q < kShards; ++q) v += cnt[(size_t)q * (T + 1) + k];
        return v;
    };
    for (int k = a; k < b; ++k) {
        const uint32_t g = tcount(gcnt, k), sm = tcount(scnt, k);
        sum.x += g;
        sum.y += sm;
        sum.z += g ? (sm + kRefUnit - 1) / kRefUnit : 0u;  // forward units: sample chunks of tiles with Gaussians
        sum.w += sm ? (g + kRefUnit - 1) / kRefUnit : 0u;  // backward units: list chunks of tiles with samples
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {  // inclusive Hillis-Steele scan of the thread partials
        const uint4 o = t >= d ? part[t - d] : make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        part[t] = make_uint4(part[t].x + o.x, part[t].y + o.y, part[t].z + o.z, part[t].w + o.w);
        __syncthreads();
    }
    const uint4 incl = part[t];
    uint32_t acc[4] = {incl.x - sum.x, incl.y - sum.y, incl.z - sum.z, incl.w - sum.w};
    uint32_t *tab[4] = {rtab + kRtGStart * (T + 1), rtab + kRtSStart * (T + 1), rtab + kRtFwdUnits * (T + 1),
                        rtab + kRtBwdUnits * (T + 1)};
    for (int k = a; k < b; ++k) {
        const uint32_t g = tcount(gcnt, k), sm = tcount(scnt, k);
        granges[k] = g ? make_uint2(acc[0], acc[0] + g) : make_uint2(0u, 0u);
        sranges[k] = sm ? make_uint2(acc[1], acc[1] + sm) : make_uint2(0u, 0u);
        for (int q = 0; q < 4; ++q) tab[q][k] = acc[q];
        acc[0] += g;
        acc[1] += sm;
        acc[2] += g ? (sm + kRefUnit - 1) / kRefUnit : 0u;
        acc[3] += sm ? (g + kRefUnit - 1) / kRefUnit : 0u;
    }
    if (t == nt - 1) {  // the totals
        tab[0][T] = incl.x; tab[1][T] = incl.y; tab[2][T] = incl.z; tab[3][T] = incl.w;
    }
}

// Copies up to 4 word arrays in one launch (the binned tensors, kept for the per-call check).
struct CopySpec {
    const uint32_t *src[4];
    uint32_t *dst[4];
    int64_t n[4];  // words
    int count;
};

// The binning's last launch: block 0 the reference-layout ranges and the call-time tables
// (ref_tables_block), the last block the headers of both buffers, every block its share of the
// binned-tensor copies (three launches before).
struct TailSpec {
    int T;
    const uint32_t *gcnt, *scnt;
    uint2 *granges, *sranges;
    uint32_t *rtab;
    char *gbuf, *sbuf;
    // the graph-capturable binning (capture != 0, dgs_bin_options.capacity_E > 0): the headers'
    // counts come from the device totals ([0] R, [1] E, [4] sort-path entries), clamped to the
    // capacities the lists were sized for; the status word (bits: 1 E, 2 sort-path entries, 4 R
    // over capacity, 8 the samples' own tile grid differs from the given one) and num_rendered
    // go to the caller; a non-zero status sets the header's "inputs differ" word, so the render
    // kernels of binned calls leave their outputs untouched (k_verify ORs it in for the others)
    int capture, D;
    const int64_t *totals;
    int64_t Rcap, Ecap, Escap;
    const int *dgrid;
    const float *doff;
    int grid[2];
    float off[2];
    int64_t *R_out;
    uint32_t *status;
    int sticky;  // DGS_BIN_STATUS_STICKY: OR into *status (it records every replay's overflows)
};

__global__ __launch_bounds__(kBlock) void k_binning_tail(CopySpec c, TailSpec ts, Header h) {
    if (blockIdx.x == 0) ref_tables_block(ts.T, ts.gcnt, ts.scnt, ts.granges, ts.sranges, ts.rtab);
    if (blockIdx.x == gridDim.x - 1) {
        const char *src = reinterpret_cast<const char *>(&h);
        for (int i = threadIdx.x; i < (int)sizeof(Header); i += blockDim.x) {
            ts.gbuf[i] = src[i];
            ts.sbuf[i] = src[i];
        }
        if (ts.capture) {
            __syncthreads();
            if (threadIdx.x == 0) {
                const int64_t R = ts.totals[0], E = ts.totals[1], Es = ts.totals[4];
                uint32_t st = (E > ts.Ecap ? 1u : 0u) | (Es > ts.Escap ? 2u : 0u) | (R > ts.Rcap ? 4u : 0u);
                for (int d = 0; ts.dgrid && d < ts.D; ++d)
                    if (ts.dgrid[d] != ts.grid[d] || __float_as_uint(ts.doff[d]) != __float_as_uint(ts.off[d])) st |= 8u;
                for (char *b : {ts.gbuf, ts.sbuf}) {
                    Header *hh = reinterpret_cast<Header *>(b);
                    hh->R = min(R, ts.Rcap);
                    hh->E = min(E, ts.Ecap);
                    hh->Es = min(Es, ts.Escap);
                    hh->zero[0] = st ? 1u : 0u;
                }
                *ts.R_out = R;
                *ts.status = ts.sticky ? (*ts.status | st) : st;
            }
        }
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
    for (int r = 0; r < c.count; ++r) {
        int64_t done = 0;
        if (((reinterpret_cast<uintptr_t>(c.src[r]) | reinterpret_cast<uintptr_t>(c.dst[r])) & 15) == 0) {
            const int64_t n4 = c.n[r] >> 2;  // 16-byte pieces
            const uint4 *s4 = reinterpret_cast<const uint4 *>(c.src[r]);
            uint4 *d4 = reinterpret_cast<uint4 *>(c.dst[r]);
            for (int64_t i = t; i < n4; i += st) d4[i] = s4[i];
            done = n4 << 2;
        }
        for (int64_t i = done + t; i < c.n[r]; i += st) c.dst[r][i] = c.src[r][i];
    }
}

// The sample side of an earlier binning of the same samples on the same grid and fine cells
// (dgs_bin_options.samples_binned): its regions copied (up to 8 word arrays), and per cell what
// the skipped launches (k_sample_cells, the sample sort, k_identify, k_sub_box) also leave in
// scratch: the tiles' sample counts (stile, for ref_tables_block's sample ranges and call-time
// tables) and the fallback-cell bits (fbg).
struct ReuseSpec {
    const uint32_t *src[8];
    uint32_t *dst[8];
    int64_t n[8];  // words
    int count;
    const int32_t *sbeg, *send;  // the source's cell ranges
    int ncells, CT, T;
    uint32_t *stile, *fbg;
};
__global__ __launch_bounds__(kBlock) void k_sample_reuse(ReuseSpec r) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
    for (int k = 0; k < r.count; ++k) {
        int64_t done = 0;
        if (((reinterpret_cast<uintptr_t>(r.src[k]) | reinterpret_cast<uintptr_t>(r.dst[k])) & 15) == 0) {
            const int64_t n4 = r.n[k] >> 2;
            const uint4 *s4 = reinterpret_cast<const uint4 *>(r.src[k]);
            uint4 *d4 = reinterpret_cast<uint4 *>(r.dst[k]);
            for (int64_t i = t; i < n4; i += st) d4[i] = s4[i];
            done = n4 << 2;
        }
        for (int64_t i = done + t; i < r.n[k]; i += st) r.dst[k][i] = r.src[k][i];
    }
    // per tile (a block each, grid-strided): its sample count into copy 0 of stile (the others
    // stay zero-filled) and its fallback cell's bit.  (Per-cell atomics put ~1.7k adds on each
    // copy's one cache line: 41 us for this launch at the headline.)
    __shared__ uint32_t part[kBlock / kWave];
    for (int tile = blockIdx.x; tile < r.T; tile += gridDim.x) {
        const int64_t c0 = (int64_t)tile * r.CT;
        uint32_t sum = 0;
        for (int k = threadIdx.x; k < r.CT; k += blockDim.x) sum += (uint32_t)(r.send[c0 + k] - r.sbeg[c0 + k]);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < (int)(blockDim.x / kWave); ++w) tot += part[w];
            r.stile[tile] = tot;
            const int64_t fb = c0 + r.CT - 1;
            set_fb_bit((int)fb, r.CT, r.send[fb] > r.sbeg[fb], r.fbg);
        }
        __syncthreads();
    }
}

// Means and conics in internal order (the forward/backward read them coalesced from here).
// Also stores perm (internal -> caller id) and its inverse back to back in gperm (one pass
// over the permutation instead of two launches).
__global__ void k_geo_pack(int P, const uint32_t *__restrict__ perm, const float2 *__restrict__ igm,
                           const float4 *__restrict__ igc, const uint64_t *__restrict__ toffs,
                           const uint64_t *__restrict__ foffs, const uint64_t *__restrict__ fcount,
                           float2 *__restrict__ gmean, float4 *__restrict__ gcon, int32_t *__restrict__ gperm,
                           uint32_t *__restrict__ rref, uint32_t *__restrict__ goff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int64_t g = perm[i];
    gperm[i] = (int32_t)g;
    gperm[P + g] = (int32_t)i;
    gmean[i] = igm[i];  // (k_fine_count's internal-order copies: coalesced, no second gather)
    const float4 c = igc[i];
    gcon[i] = make_float4(c.x, c.y, c.z, 0.0f);
    // rlist's inputs (ensure_ref_lists): the tile-list offsets in caller order, copied coalesced
    // (toffs < R < 2^31 when the binning succeeds; preprocess fails otherwise), then the radii
    // in internal order
    rref[i] = (uint32_t)toffs[i];
    rref[P + i] = __float_as_uint(c.w);
    // the Gaussian-major slots of the sort-path entries (k_fine_fill's offsets; < 2^31)
    goff[i] = (uint32_t)foffs[i];
    if (i == P - 1) goff[P] = (uint32_t)(foffs[i] + fcount[i]);
}

// Forward sample pair rows in sorted order: pair p = samples 2p, 2p+1, field-interleaved
// [s0 s0' (s1 s1')]; a missing second sample (odd N) is 0 (zero-filled with phase A).  Written by
// the sample sort's last place (FsRows: the payload of dgs_radix.h's Extra hook).
struct FsRows {
    const float *samples;
    float *rows;
    int D;
    __device__ __forceinline__ void operator()(uint32_t j, uint32_t sid) const {
        float *row = rows + (int64_t)(j >> 1) * (2 * D) + (j & 1);
        row[0] = samples[(int64_t)sid * D];
        if (D == 2) row[2] = samples[(int64_t)sid * D + 1];
    }
};


// Zero-fills up to kZeroMax word-aligned regions in one launch (each hipMemsetAsync is a launch
// of its own, ~5 us of GPU time even for a few bytes; the binning needs eleven).
constexpr int kZeroMax = 20;
struct ZeroSpec {
    uint32_t *p[kZeroMax];
    int64_t n[kZeroMax];  // words
    int count;
};

__global__ void k_zero_multi(ZeroSpec z) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
    for (int r = 0; r < z.count; ++r)
        for (int64_t i = t; i < z.n[r]; i += st) z.p[r][i] = 0u;
}

struct ZeroList {
    ZeroSpec z{};
    bool overflow = false;
    void add(void *p, size_t bytes) {
        if (z.count >= kZeroMax) { overflow = true; return; }
        z.p[z.count] = static_cast<uint32_t *>(p);
        z.n[z.count++] = (int64_t)(bytes / 4);
    }
    hipError_t launch(hipStream_t s) {
        if (overflow) return hipErrorInvalidValue;  // (a programming error: raise kZeroMax)
        k_zero_multi<<<256, 256, 0, s>>>(z);
        return hipGetLastError();
    }
};

static inline unsigned grid_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// Every sort of the binning is dgs_radix.h's stable LSD radix sort of (key, u32 value) pairs.
// Entry keys are u16 when every (cell, flag) key fits 16 bits (6 instead of 8 bytes moved per
// entry and place).

// Chooses the fine subdivision: about 120 samples per fine cell on average (two forward
// waves per cell), capped so that cells stay reasonably large for sparse sample sets.
// Fine cells per tile axis.  A forward unit holds up to kFwdUnit = 128 samples of one cell and
// walks the cell's whole Gaussian list, so the mean cell population is set a few Poisson
// deviations below 128 (a cell just over 128 pays a second full walk for a few samples);
// smaller cells also cull more.  DGS_CELL_TARGET overrides the mean (tuning).
static double cell_target() {
    static const double t = [] {
        const char *e = std::getenv("DGS_CELL_TARGET");
        const double v = e ? std::atof(e) : 0.0;
        return v > 0.0 ? v : 150.0;
    }();
    return t;
}

// area > 0: the samples occupy `area` (D = 2; a length at D = 1) of the domain, e.g. one
// rank's strip of a spatially sharded run -- the density is N / area, not N / (T tiles).
static int choose_n(int D, int64_t N, int64_t T, double area) {
    const double tile_area = D == 2 ? (double)kTile * (double)kTile : (double)kTile;
    const double per_tile = area > 0.0 ? (double)N * tile_area / area : (double)N / (double)(T > 0 ? T : 1);
    const double target = cell_target();
    if (D == 2) {
        int n = (int)std::lround(std::sqrt(per_tile / target));
        return std::max(1, std::min(n, 64));
    }
    int n = (int)std::lround(per_tile / target);
    return std::max(1, std::min(n, 1 << 16));
}

// Scratch carving: the pieces of one phase are planned as offsets (fake pointers), then taken
// from ONE callback allocation and rebased -- each callback is a torch allocation on the host
// (~5-10 us), and after the host sync the GPU idles while the host allocates.
struct Carve {
    size_t off = 0;
    template <typename T>
    T *take(size_t count) {
        const size_t o = off;
        off = align_up(off + std::max<size_t>(count * sizeof(T), 16), 256);
        return reinterpret_cast<T *>(o + 256);  // +256: no planned piece is a null pointer
    }
    template <typename T>
    static void rebase(T *&p, char *base) {
        p = reinterpret_cast<T *>(base + (reinterpret_cast<uintptr_t>(p) - 256));
    }
};

// Scratch allocator: every piece comes from the caller's callback.
struct Scratch {
    dgs_alloc_fn fn;
    void *ctx;
    int rc = DGS_OK;
    template <typename T>
    T *get(size_t count) {
        if (rc) return nullptr;
        void *p = fn(ctx, DGS_BUF_SCRATCH, align_up(std::max<size_t>(count * sizeof(T), 16), 256));
        if (!p) rc = fail(DGS_ERR_ALLOC, "scratch allocation failed");
        return static_cast<T *>(p);
    }
};


// ------------------------------------------------------------ spatial shards
// Per Gaussian, the ranks whose point range along the sharding axis (y at D = 2, x at D = 1)
// meets its exact-zero cut X^T A X <= kQCut or a torus image of it (period 2,
// forward.cu:149-157): bit r of mask[g]; and the owner, the rank whose range is nearest the mean
// (first on ties) among the ranks it touches, the nearest of all if it touches none.  The cut's half-width along the axis is sqrt(kQCut (A^-1)_axis), widened by
// 1e-5; conics that are not positive definite reach every rank.
constexpr int kMaxXchgRanks = 32;
struct XchgRanks {
    int W;
    double lo[kMaxXchgRanks], hi[kMaxXchgRanks];
};

__global__ void k_xchg_sets(int P, int D, const float *__restrict__ means, const float *__restrict__ conics,
                            XchgRanks R, uint32_t *__restrict__ mask, int32_t *__restrict__ owner) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P) return;
    const int S = D * (D + 1) / 2;
    const double y = means[g * D + (D - 1)];
    double e;
    bool pd;
    if (D == 2) {
        const double c0 = conics[g * S], c1 = conics[g * S + 1], c2 = conics[g * S + 2];
        const double det = c0 * c2 - c1 * c1;
        pd = c0 > 0.0 && det > 0.0 && det < INFINITY && c0 < INFINITY && c2 < INFINITY &&
             c1 * c1 < kRho2Max * (c0 * c2);  // (the binning's cut: gauss_cut)
        e = pd ? sqrt(kQCut * c0 / det) : INFINITY;
    } else {
        const double c0 = conics[g * S];
        pd = c0 > 0.0 && c0 < INFINITY;
        e = pd ? sqrt(kQCut / c0) : INFINITY;
    }
    e = e * (1.0 + 1e-5) + 1e-6;
    uint32_t m = 0u;
    int best = 0, tbest = -1;
    double bd = INFINITY, tbd = INFINITY;
    for (int r = 0; r < R.W; ++r) {
        const double lo = R.lo[r], hi = R.hi[r];
        if (!pd) {
            m |= 1u << r;
        } else {  // some k with [y + 2k - e, y + 2k + e] meeting [lo, hi]
            const double kmin = ceil((lo - y - e) * 0.5), kmax = floor((hi - y + e) * 0.5);
            if (kmin <= kmax) m |= 1u << r;
        }
        const double d = fmax(fmax(lo - y, y - hi), 0.0);
        if (d < bd) { bd = d; best = r; }
        if (((m >> r) & 1u) && d < tbd) { tbd = d; tbest = r; }
    }
    mask[g] = m;
    owner[g] = tbest >= 0 ? tbest : best;  // a rank that touches it; the nearest if none does
}
}  // namespace dgs

using namespace dgs;

extern "C" const char *dgs_last_error(void) { return g_last_error.c_str(); }
extern "C" int64_t dgs_internal_allocations(void) { return g_internal_allocs.load(std::memory_order_relaxed); }
extern "C" int dgs_version(void) { return (int)kVersion; }

namespace dgs {
hipError_t warm_preprocess(hipStream_t);
hipError_t warm_sample(hipStream_t);
hipError_t warm_aggregate(hipStream_t);
hipError_t warm_volume(hipStream_t);
hipError_t warm_reference(hipStream_t);
}  // namespace dgs

extern "C" int dgs_warmup(dgs_stream_t stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (hipError_t (*w)(hipStream_t) : {dgs::warm_preprocess, dgs::warm_sample, dgs::warm_aggregate,
                                         dgs::warm_volume, dgs::warm_reference})
        DGS_TRY_HIP(w(s));
    DGS_TRY_HIP(hipStreamSynchronize(s));
    return DGS_OK;
}

extern "C" int dgs_tile_grid(int N, int D, const float *samples, int *grid_out, float *off_out,
                             dgs_stream_t stream) {
    if (N <= 0 || (D != 1 && D != 2) || !samples) return fail(DGS_ERR_ARG, "dgs_tile_grid: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nparts = (int)std::min<int64_t>(1024, grid_for(N));
    float *part = nullptr;
    int *dgrid = nullptr;
    float *doff = nullptr;
    note_internal_alloc();  // (dgs_tile_grid's scratch: dgs.h)
    DGS_TRY_HIP(hipMallocAsync(&part, sizeof(float) * 4 * nparts, s));
    DGS_TRY_HIP(hipMallocAsync(&dgrid, sizeof(int) * 2, s));
    DGS_TRY_HIP(hipMallocAsync(&doff, sizeof(float) * 2, s));
    k_bounds_partial<<<nparts, kBlock, 0, s>>>(N, D, samples, part);
    k_bounds_final<<<1, kBlock, 0, s>>>(nparts, D, part, dgrid, doff);
    DGS_TRY_HIP(hipGetLastError());
    int hg[2];
    float ho[2];
    DGS_TRY_HIP(hipMemcpyAsync(hg, dgrid, sizeof(int) * D, hipMemcpyDeviceToHost, s));
    DGS_TRY_HIP(hipMemcpyAsync(ho, doff, sizeof(float) * D, hipMemcpyDeviceToHost, s));
    DGS_TRY_HIP(hipStreamSynchronize(s));
    DGS_TRY_HIP(hipFreeAsync(part, s));
    DGS_TRY_HIP(hipFreeAsync(dgrid, s));
    DGS_TRY_HIP(hipFreeAsync(doff, s));
    for (int d = 0; d < D; ++d) { grid_out[d] = hg[d]; off_out[d] = ho[d]; }
    return DGS_OK;
}

namespace dgs {
// Entry / tile-list sizes of the previous binning of the same (P, N, D): the capacities the
// next call allocates before its host sync (PhaseB in preprocess_body).
struct SizeSpec {
    int64_t E = -1, R = -1;
};
static std::mutex g_spec_mu;
static int64_t g_spec_key[3] = {-1, -1, -1};
static SizeSpec g_spec;
static SizeSpec size_spec_get(int P, int N, int D) {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    return (g_spec_key[0] == P && g_spec_key[1] == N && g_spec_key[2] == D) ? g_spec : SizeSpec{};
}
static void size_spec_put(int P, int N, int D, int64_t E, int64_t R) {
    std::lock_guard<std::mutex> lk(g_spec_mu);
    g_spec_key[0] = P; g_spec_key[1] = N; g_spec_key[2] = D;
    g_spec.E = E;
    g_spec.R = R;
}

// DGS_QCUT_REFERENCE=1 (read once): every binning of the process as with DGS_BIN_QCUT_REFERENCE.
static bool qcut_reference_env() {
    static const bool on = [] {
        const char *e = std::getenv("DGS_QCUT_REFERENCE");
        return e && e[0] && e[0] != '0';
    }();
    return on;
}

// The binning with the host-known grid `grid`/`grid_offset`.  dgrid/doff (device, optional): a
// device-computed grid read back at the one host sync into *dev_grid / *dev_off (D entries).
static int preprocess_body(int P, int D, int N, const float *means, const float *covariances,
                           const float *conics, const float *samples, const int *grid,
                           const float *grid_offset, float *radii, dgs_alloc_fn alloc,
                           void *alloc_ctx, int64_t *num_rendered, dgs_stream_t stream, int debug,
                           const int *dgrid, const float *doff, int *dev_grid, float *dev_off,
                           const uint8_t *present = nullptr, double sample_area = 0.0,
                           const dgs_bin_options *copt = nullptr, bool own_grid = false) {
    // the graph-capturable form (dgs.h, dgs_bin_options.capacity_E > 0): no host sync and no
    // host read of a device value -- the lists are sized from the caller's capacities, the exact
    // counts stay on the device (capacity-sized launches read them), overflows are reported in
    // the status word (k_binning_tail)
    const bool capmode = copt && copt->capacity_E > 0;
    if (D != 1 && D != 2) return fail(DGS_ERR_ARG, "only D = 1 or D = 2 is supported (the reference leaves D = 3 undefined)");
    if (P < 0 || N < 0 || !alloc || !num_rendered) return fail(DGS_ERR_ARG, "dgs_preprocess: bad arguments");
    if ((int64_t)P > kMaxGaussians) return fail(DGS_ERR_ARG, "too many Gaussians (limit 2^29 - 1)");
    *num_rendered = 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (capmode) {
        if (!copt->num_rendered_device || !copt->status_device || copt->capacity_R <= 0 || copt->capacity_Es < 0)
            return fail(DGS_ERR_ARG, "dgs_preprocess_ex: the capturable binning needs capacity_R > 0, "
                                     "capacity_Es >= 0, num_rendered_device and status_device");
        *num_rendered = -1;  // (on the device: *num_rendered_device)
        if (P == 0 || N == 0) {  // sample_points.cu:69: nothing to bin
            DGS_TRY_HIP(hipMemsetAsync(copt->num_rendered_device, 0, sizeof(int64_t), s));
            if (!(copt->flags & DGS_BIN_STATUS_STICKY))
                DGS_TRY_HIP(hipMemsetAsync(copt->status_device, 0, sizeof(uint32_t), s));
            return DGS_OK;
        }
    }
    if (P == 0 || N == 0) return DGS_OK;  // sample_points.cu:69: nothing to bin
    if (!grid || !grid_offset) return fail(DGS_ERR_ARG, "dgs_preprocess: grid/offset required");

    Geom G;
    G.D = D;
    G.grid[0] = grid[0];
    G.grid[1] = D == 2 ? grid[1] : 1;
    G.off[0] = grid_offset[0];
    G.off[1] = D == 2 ? grid_offset[1] : 0.0f;
    if (G.grid[0] <= 0 || G.grid[1] <= 0) return fail(DGS_ERR_ARG, "tile grid must be positive");
    const int64_t T64 = (int64_t)G.grid[0] * G.grid[1];
    if (T64 > (1 << 24)) return fail(DGS_ERR_ARG, "tile grid too large");
    G.T = (int)T64;
    G.n = choose_n(D, N, G.T, sample_area);
    G.CT = (D == 2 ? G.n * G.n : G.n) + 1;
    const int64_t ncells64 = (int64_t)G.T * G.CT;
    if (ncells64 >= (1LL << 30)) return fail(DGS_ERR_ARG, "too many fine cells");
    G.ncells = (int)ncells64;
    G.fs = (double)kTile / G.n;
    G.ifs = 1.0 / G.fs;
    // (the A/B and test knob: every entry binned with the reference cut, as before kQCutFast)
    const bool ref_cut = (copt && (copt->flags & DGS_BIN_QCUT_REFERENCE)) || qcut_reference_env();
    G.qf = ref_cut ? kQCut : kQCutFast;
    G.rf = ref_cut ? 1.0 : std::sqrt(kQCutFast / kQCut);
    const int ncells = G.ncells;
    const int home_w = G.grid[0] * G.n, home_h = D == 2 ? G.grid[1] * G.n : 1;
    // an earlier binning of the same samples on this grid and these fine cells: its sample side
    UnitHint prev;
    const bool reuse = copt && copt->samples_binned && (!capmode || (copt->flags & DGS_BIN_SAMPLES_FIXED)) &&
                       hint_by_sbuf(copt->samples_binned, copt->samples_binned_bytes, &prev) &&
                       prev.hdr.N == N && prev.hdr.D == D && prev.hdr.T == G.T && prev.hdr.n == G.n &&
                       prev.hdr.CT == G.CT && prev.hdr.ncells == G.ncells && prev.hdr.grid[0] == G.grid[0] &&
                       prev.hdr.grid[1] == G.grid[1] && std::memcmp(prev.hdr.off, G.off, sizeof(G.off)) == 0;

    // ---- sample-side buffer (size known now) and the reference range buffers
    const int64_t fwd_cap = (N + kFwdUnit - 1) / kFwdUnit + 2 * std::min<int64_t>(N, ncells) + 1;
    Layout L0 = make_layout(D, P, N, G.T, 0, ncells, 0, fwd_cap, 0);
    char *sbuf = static_cast<char *>(alloc(alloc_ctx, DGS_BUF_SAMPLE_BINNING, L0.s_bytes));
    char *rbuf = static_cast<char *>(alloc(alloc_ctx, DGS_BUF_RANGES, (size_t)G.T * 8 + 8));
    char *srbuf = static_cast<char *>(alloc(alloc_ctx, DGS_BUF_SAMPLE_RANGES, (size_t)G.T * 8 + 8));
    if (!sbuf || !rbuf || !srbuf) return fail(DGS_ERR_ALLOC, "buffer allocation failed");
    int32_t *sorted_sid = reinterpret_cast<int32_t *>(sbuf + L0.o_sorted);
    float4 *cell_box = reinterpret_cast<float4 *>(sbuf + L0.o_cell_box);
    int32_t *cell_sbeg = reinterpret_cast<int32_t *>(sbuf + L0.o_cell_sbeg);
    int32_t *cell_send = reinterpret_cast<int32_t *>(sbuf + L0.o_cell_send);
    uint2 *fwd_units = reinterpret_cast<uint2 *>(sbuf + L0.o_fwd_units);
    const int nsub = D == 2 ? kSubPerCell * ncells : 0;
    int32_t *sub_sbeg = reinterpret_cast<int32_t *>(sbuf + L0.o_sub_sbeg);
    int32_t *sub_send = reinterpret_cast<int32_t *>(sbuf + L0.o_sub_send);
    float4 *sub_box = reinterpret_cast<float4 *>(sbuf + L0.o_sub_box);
    uint2 *fsub_units = reinterpret_cast<uint2 *>(sbuf + L0.o_fsub_units);

    Scratch S{alloc, alloc_ctx};
    Carve ca;
    uint32_t *skeys = ca.take<uint32_t>(N), *skeys_sorted = ca.take<uint32_t>(N), *sids = ca.take<uint32_t>(N);
    // (tile counts, largest reach and entry counts: kShards copies each, see kShards)
    const size_t tcw = (size_t)kShards * (G.T + 1);
    uint32_t *stile = ca.take<uint32_t>(tcw), *gtile = ca.take<uint32_t>(tcw);
    uint32_t *home = ca.take<uint32_t>(P), *home_sorted = ca.take<uint32_t>(P), *gids = ca.take<uint32_t>(P);
    uint32_t *perm = ca.take<uint32_t>(P);
    uint64_t *touched = ca.take<uint64_t>(P), *fcount = ca.take<uint64_t>(P), *foffs = ca.take<uint64_t>(P);
    uint64_t *toffs = ca.take<uint64_t>(P);
    int64_t *totals = ca.take<int64_t>(8);
    const int HK = home_w * home_h;  // (home cell keys; HK = absent)
    int8_t *greach = ca.take<int8_t>(P);
    uint32_t *lrows = ca.take<uint32_t>((size_t)kGatherRows * P);
    uint32_t *hstart = ca.take<uint32_t>((size_t)HK + 1), *gcnt = ca.take<uint32_t>(ncells);
    uint32_t *cnt2 = ca.take<uint32_t>((size_t)kGatherRows * ncells);
    uint32_t *fbg = ca.take<uint32_t>((size_t)(G.T + 31) / 32 + 2);  // fallback-cell bits (+2: fb_load's words)
    // k_fine_count's queue: kShards parts of qcap ids (a part takes the blocks b = s mod kShards)
    const int qcap = (int)((grid_for(P) + kShards - 1) / kShards) * kBlock;
    uint32_t *irr = ca.take<uint32_t>((size_t)kShards * qcap), *nirr = ca.take<uint32_t>(kShards * kShard32);
    uint32_t *wq = ca.take<uint32_t>(P), *nwq = ca.take<uint32_t>(kShard32);  // k_wide's queue
    uint2 *irect = ca.take<uint2>(P);  // reference rects in internal order
    unsigned long long *eg = ca.take<unsigned long long>(kShards * kShard64);  // per copy [gathered, kUnsafe, kThin entries]
    int32_t *rmax = ca.take<int32_t>(kShards * kShard32);
    float2 *igm = ca.take<float2>(P);
    float4 *igc = ca.take<float4>(P);
    float4 *grec = ca.take<float4>(2 * (size_t)P);
    unsigned long long *fscan_a = ca.take<unsigned long long>(fused_scan_state_words(P, 2, 8));
    // capturable binning: the samples' own tile grid (sample_points.cu:70-74), checked on the device
    const int nparts = capmode ? (int)std::min<int64_t>(1024, grid_for(N)) : 1;
    float *bpart = ca.take<float>(4 * (size_t)nparts);
    int32_t *cgrid = ca.take<int32_t>(4);
    float *coff = ca.take<float>(4);

    // the two phase-A sorts' scratch (each with its own zero-filled head: see dgs_radix.h)
    const int sbits = bit_length((uint64_t)ncells * kSubPerCell);  // (cell, sub-cell) keys
    const int hbits = bit_length((uint64_t)home_w * (uint64_t)home_h);  // absent key = home_w * home_h
    const RadixPlan plan_s = radix_plan(N, sbits), plan_h = radix_plan(P, hbits);
    char *rs_s = ca.take<char>(plan_s.bytes), *rs_h = ca.take<char>(plan_h.bytes);
    {
        char *base = S.get<char>(ca.off);
        if (S.rc) return S.rc;
        for (uint32_t **q : {&skeys, &skeys_sorted, &sids, &stile, &gtile, &home, &home_sorted, &gids, &perm})
            Carve::rebase(*q, base);
        for (uint64_t **q : {&touched, &fcount, &foffs, &toffs}) Carve::rebase(*q, base);
        Carve::rebase(totals, base);
        Carve::rebase(greach, base);
        Carve::rebase(lrows, base);
        Carve::rebase(cnt2, base);
        Carve::rebase(fbg, base);
        Carve::rebase(irr, base);
        Carve::rebase(nirr, base);
        Carve::rebase(wq, base);
        Carve::rebase(nwq, base);
        Carve::rebase(irect, base);
        Carve::rebase(hstart, base);
        Carve::rebase(gcnt, base);
        Carve::rebase(eg, base);
        Carve::rebase(rmax, base);
        Carve::rebase(igm, base);
        Carve::rebase(igc, base);
        Carve::rebase(grec, base);
        Carve::rebase(fscan_a, base);
        Carve::rebase(bpart, base);
        Carve::rebase(cgrid, base);
        Carve::rebase(coff, base);
        Carve::rebase(rs_s, base);
        Carve::rebase(rs_h, base);
    }

    float *fsrows = reinterpret_cast<float *>(sbuf + L0.o_fsrows);
    {  // one launch for every zero-fill of phase A (the sample sort writes fsrows but its slack)
        const size_t fs_written = (size_t)(N / 2 * 2) * D * 4;  // (the sort writes whole pairs; an odd N's last one from here)
        ZeroList zl;
        zl.add(stile, sizeof(uint32_t) * tcw);
        zl.add(gtile, sizeof(uint32_t) * tcw);
        zl.add(cell_sbeg, sizeof(int32_t) * ncells);
        zl.add(cell_send, sizeof(int32_t) * ncells);
        if (nsub) {
            zl.add(sub_sbeg, sizeof(int32_t) * nsub);
            zl.add(sub_send, sizeof(int32_t) * nsub);
        }
        zl.add(reinterpret_cast<char *>(fsrows) + fs_written, fsrows_bytes(N, D) - fs_written);
        zl.add(rbuf, (size_t)G.T * 8 + 8);
        zl.add(srbuf, (size_t)G.T * 8 + 8);
        zl.add(cnt2, sizeof(uint32_t) * kGatherRows * (size_t)ncells);
        zl.add(eg, 8 * kShards * kShard64);
        zl.add(fscan_a, 8 * fused_scan_state_words(P, 2, 8));
        zl.add(rmax, 4 * kShards * kShard32);
        zl.add(fbg, sizeof(uint32_t) * ((size_t)(G.T + 31) / 32 + 2));
        zl.add(nirr, 4 * kShards * kShard32);
        zl.add(nwq, 4 * kShard32);
        zl.add(rs_s, plan_s.zero_bytes);
        zl.add(rs_h, plan_h.zero_bytes);
        DGS_TRY_HIP(zl.launch(s));
        DGS_LAUNCH_CHECK(s, debug);
    }

    if (capmode && !reuse) {  // (fixed samples: their grid is the reused binning's)
        k_bounds_partial<<<nparts, kBlock, 0, s>>>(N, D, samples, bpart);
        k_bounds_final<<<1, kBlock, 0, s>>>(nparts, D, bpart, cgrid, coff);
        DGS_LAUNCH_CHECK(s, debug);
    }
    if (reuse) {  // ---- samples: copied from the earlier binning of the same samples
        const Header &ph = prev.hdr;
        const char *ps = static_cast<const char *>(prev.sbuf);
        ReuseSpec r{};
        const auto add = [&](int64_t so, int64_t dofs, size_t bytes) {
            r.src[r.count] = reinterpret_cast<const uint32_t *>(ps + so);
            r.dst[r.count] = reinterpret_cast<uint32_t *>(sbuf + dofs);
            r.n[r.count] = (int64_t)(bytes / 4);
            ++r.count;
        };
        add(ph.o_sorted, L0.o_sorted, sizeof(int32_t) * (size_t)N);
        add(ph.o_cell_box, L0.o_cell_box, sizeof(float4) * (size_t)ncells);
        add(ph.o_cell_sbeg, L0.o_cell_sbeg, sizeof(int32_t) * (size_t)ncells);
        add(ph.o_cell_send, L0.o_cell_send, sizeof(int32_t) * (size_t)ncells);
        add(ph.o_fsrows, L0.o_fsrows, fsrows_bytes(N, D));
        if (nsub) {
            add(ph.o_sub_sbeg, L0.o_sub_sbeg, sizeof(int32_t) * (size_t)nsub);
            add(ph.o_sub_send, L0.o_sub_send, sizeof(int32_t) * (size_t)nsub);
            add(ph.o_sub_box, L0.o_sub_box, sizeof(float4) * (size_t)nsub);
        }
        r.sbeg = reinterpret_cast<const int32_t *>(ps + ph.o_cell_sbeg);
        r.send = reinterpret_cast<const int32_t *>(ps + ph.o_cell_send);
        r.ncells = ncells;
        r.CT = G.CT;
        r.T = G.T;
        r.stile = stile;
        r.fbg = fbg;
        k_sample_reuse<<<1024, kBlock, 0, s>>>(r);
        DGS_LAUNCH_CHECK(s, debug);
        g_sample_reuse.fetch_add(1, std::memory_order_relaxed);
    } else {
    // ---- samples: fine cell keys, stable radix sort, per-cell ranges
    k_sample_cells<<<hist_grid(N), kBlock, 0, s>>>(N, G, samples, skeys, sids, stile, radix_hist(plan_s, rs_s));
    DGS_LAUNCH_CHECK(s, debug);
    DGS_TRY_HIP(radix_sort<uint32_t>(plan_s, N, rs_s, skeys, skeys_sorted, sids, reinterpret_cast<uint32_t *>(sorted_sid),
                                     s, true, FsRows{samples, fsrows, D}));
    DGS_LAUNCH_CHECK(s, debug);
    k_identify<uint32_t><<<grid_for(N), kBlock, 0, s>>>(N, skeys_sorted, (uint32_t)ncells, cell_sbeg, cell_send, 2,
                                                        (uint32_t)nsub, nsub ? sub_sbeg : nullptr, sub_send, 0);
    DGS_LAUNCH_CHECK(s, debug);
    if (nsub)  // sub-cell boxes and the cell boxes (their union)
        k_sub_box<<<(unsigned)((ncells + kBlock / kWave - 1) / (kBlock / kWave)), kBlock, 0, s>>>(
            ncells, G.CT, sub_sbeg, sub_send, fsrows, sub_box, cell_box, fbg);
    else
        k_cell_box<<<(unsigned)((ncells + kBlock / kWave - 1) / (kBlock / kWave)), kBlock, 0, s>>>(
            ncells, D, G.CT, cell_sbeg, cell_send, fsrows, cell_box, fbg);
    DGS_LAUNCH_CHECK(s, debug);
    }

    // ---- Gaussians: reference radius/touched, spatial renumbering, fine entry counts
    k_gauss_prep<<<hist_grid(P), kBlock, 0, s>>>(P, G, means, covariances, conics, radii, touched, gtile,
                                                home, gids, home_w, home_h, present, grec, radix_hist(plan_h, rs_h));
    DGS_LAUNCH_CHECK(s, debug);
    DGS_TRY_HIP(radix_sort<uint32_t>(plan_h, P, rs_h, home, home_sorted, gids, perm, s, true));
    DGS_LAUNCH_CHECK(s, debug);
    k_gauss_permute<<<grid_for(P), kBlock, 0, s>>>(P, perm, grec, igm, igc, irect);
    DGS_LAUNCH_CHECK(s, debug);
    k_fine_count<<<grid_for(P), kBlock, 0, s>>>(P, G, igm, igc, irect, fbg, fcount, greach, lrows, rmax, irr, nirr,
                                                qcap, eg + 1);
    DGS_LAUNCH_CHECK(s, debug);
    k_fine_count_irr<<<std::min(grid_for(P), 2048u), kBlock, 0, s>>>(G, igm, igc, cell_sbeg, cell_send, cell_box, fbg,
                                                                     greach, irr, nirr, qcap, fcount, eg + 1, wq, nwq);
    DGS_LAUNCH_CHECK(s, debug);
    k_wide<false, uint32_t><<<kWideBlocks, kBlock, 0, s>>>(G, igm, igc, cell_sbeg, cell_send, cell_box, fbg, wq, nwq,
                                                           fcount, nullptr, nullptr, nullptr, 0, eg + 1, nullptr);
    DGS_LAUNCH_CHECK(s, debug);
    const unsigned gather_blocks = (unsigned)(((int64_t)home_h * ((home_w + kStripW - 1) / kStripW) * kGatherRows +
                                               kWavesPerBlock - 1) / kWavesPerBlock);
    if (D == 2) {  // the regular Gaussians' local entries, per cell (k_gather)
        k_home_start<<<grid_for((int64_t)HK + 1), kBlock, 0, s>>>(P, HK, home_sorted, hstart);
        DGS_LAUNCH_CHECK(s, debug);
        k_gather<false><<<gather_blocks, kBlock, 0, s>>>(G, P, greach, lrows, hstart, rmax, cnt2, eg, nullptr, nullptr);
        DGS_LAUNCH_CHECK(s, debug);
    }
    {  // sort-path entry offsets and the reference's tile-list offsets (sampler_impl.cu:253), then
       // the totals read back at the sync: R (num_rendered), E, the device grid (k_bounds_final)
       // and the gathered / kUnsafe entry counts of k_gather / k_fine_count (eg[0], eg[1])
        const uint64_t *fc = fcount, *tc = touched;
        uint64_t *fo = foffs, *to = toffs;
        const unsigned long long *egc = eg;
        int64_t *tot = totals;
        const int *dg = dgrid;
        const float *dof = doff;
        DGS_TRY_HIP((fused_scan<2, 8>(
            (int64_t)P, fscan_a,
            [=] __device__(int64_t i, uint64_t *x) { x[0] = fc[i]; x[1] = tc[i]; },
            [=] __device__(int64_t i, const uint64_t *, const uint64_t *ex) { fo[i] = ex[0]; to[i] = ex[1]; },
            [=] __device__(const uint64_t *t) {
                unsigned long long ec[3] = {0, 0, 0};  // (the counters' copies)
                for (int q = 0; q < kShards; ++q)
                    for (int k = 0; k < 3; ++k) ec[k] += egc[q * kShard64 + k];
                tot[0] = (int64_t)t[1];                  // num_rendered (sampler_impl.cu:253-257)
                tot[1] = (int64_t)t[0] + (int64_t)ec[0];  // all entries
                tot[4] = (int64_t)t[0];                  // sort-path entries
                tot[5] = (int64_t)ec[0];
                tot[6] = (int64_t)ec[1];
                tot[7] = (int64_t)ec[2];
                int32_t *g = reinterpret_cast<int32_t *>(tot + 2);
                g[0] = dg ? dg[0] : 0;
                g[1] = dg ? dg[1] : 0;
                g[2] = dof ? __float_as_int(dof[0]) : 0;
                g[3] = dof ? __float_as_int(dof[1]) : 0;
            },
            s)));
        DGS_LAUNCH_CHECK(s, debug);
    }
    // ---- Gaussian-side buffer and phase-B scratch for capacities (Ecap, Rcap).  Set up BEFORE
    // the host sync with the previous call's sizes (+1/8) when known, so the allocations and the
    // E-independent launches (k_geo_pack, the zero-fills) overlap the sync; redone after it only
    // if this call's E or R does not fit.
    struct PhaseB {
        int64_t Ecap = -1, Rcap = -1, bwd_cap = 0;
        Layout L;
        char *gbuf = nullptr;
        uint32_t *ekeys, *evals, *ekeys_sorted, *svals;
        unsigned long long *fs_cells, *fs_units, *fs_sub;  // fused_scan states (zeroed with phase B)
        int32_t *hbeg, *hend;
        char *rs_e;  // the entry sort's scratch (zero head filled with phase B's regions)
        RadixPlan plan_e;
        bool k16;
        int ebits;
    };
    auto setup_b = [&](int64_t Ecap, int64_t Rcap, PhaseB &B) -> int {
        B.Ecap = Ecap;
        B.Rcap = Rcap;
        B.bwd_cap = (Ecap + kWave - 1) / kWave + std::min<int64_t>(Ecap, ncells) + 1;
        B.L = make_layout(D, P, N, G.T, Rcap, ncells, Ecap, fwd_cap, B.bwd_cap);
        B.gbuf = static_cast<char *>(alloc(alloc_ctx, DGS_BUF_BINNING, B.L.g_bytes));
        if (!B.gbuf) return fail(DGS_ERR_ALLOC, "binning buffer allocation failed");
        Carve cb;
        B.ekeys = cb.take<uint32_t>(Ecap + 1); B.evals = cb.take<uint32_t>(Ecap + 1);
        B.ekeys_sorted = cb.take<uint32_t>(Ecap + 1); B.svals = cb.take<uint32_t>(Ecap + 1);
        B.hbeg = cb.take<int32_t>(2 * (size_t)ncells); B.hend = cb.take<int32_t>(2 * (size_t)ncells);
        B.fs_cells = cb.take<unsigned long long>(fused_scan_state_words(ncells, 1, 1));
        B.fs_units = cb.take<unsigned long long>(fused_scan_state_words(ncells, 2, 1));
        B.fs_sub = cb.take<unsigned long long>(fused_scan_state_words(std::max(nsub, 1), 1, 1));
        B.ebits = bit_length((uint64_t)(ncells > 1 ? ncells - 1 : 1)) + 2;  // + slow and thin bits
        B.k16 = B.ebits <= 16;  // (cell, flag) keys in 16 bits: a u16-key sort
        B.plan_e = radix_plan(Ecap, B.ebits);
        B.rs_e = cb.take<char>(B.plan_e.bytes);
        char *base = S.get<char>(cb.off);
        if (S.rc) return S.rc;
        for (uint32_t **q : {&B.ekeys, &B.evals, &B.ekeys_sorted, &B.svals})
            Carve::rebase(*q, base);
        for (unsigned long long **q : {&B.fs_cells, &B.fs_units, &B.fs_sub}) Carve::rebase(*q, base);
        Carve::rebase(B.hbeg, base);
        Carve::rebase(B.hend, base);
        Carve::rebase(B.rs_e, base);
        ZeroList zl;
        zl.add(B.gbuf + B.L.o_counts, 16);
        zl.add(B.hbeg, sizeof(int32_t) * 2 * (size_t)ncells);
        zl.add(B.hend, sizeof(int32_t) * 2 * (size_t)ncells);
        zl.add(B.fs_cells, 8 * fused_scan_state_words(ncells, 1, 1));
        zl.add(B.fs_units, 8 * fused_scan_state_words(ncells, 2, 1));
        zl.add(B.fs_sub, 8 * fused_scan_state_words(std::max(nsub, 1), 1, 1));
        zl.add(B.rs_e, B.plan_e.zero_bytes);
        DGS_TRY_HIP(zl.launch(s));
        DGS_LAUNCH_CHECK(s, debug);
        k_geo_pack<<<grid_for(P), kBlock, 0, s>>>(P, perm, igm, igc, toffs, foffs, fcount,
                                                  reinterpret_cast<float2 *>(B.gbuf + B.L.o_gmean),
                                                  reinterpret_cast<float4 *>(B.gbuf + B.L.o_gcon),
                                                  reinterpret_cast<int32_t *>(B.gbuf + B.L.o_perm),
                                                  reinterpret_cast<uint32_t *>(B.gbuf + B.L.o_rref),
                                                  reinterpret_cast<uint32_t *>(B.gbuf + B.L.o_goff));
        DGS_LAUNCH_CHECK(s, debug);
        return DGS_OK;
    };
    PhaseB B;
    int64_t R, E, Es;
    int64_t *htot = nullptr;
    uint32_t *herr = nullptr;
    if (capmode) {  // the caller's capacities: no sync, no read-back
        R = copt->capacity_R;
        E = copt->capacity_E;
        Es = std::min(copt->capacity_Es, E);
        if (E >= (1LL << 31) - 64) return fail(DGS_ERR_ARG, "capacity_E too large (2^31)");
        if (nsub && kSubPerCell * E >= (1LL << 31) - 64)
            return fail(DGS_ERR_ARG, "capacity_E too large for the sub-cell lists (4 E >= 2^31)");
        if (R >= (1LL << 31) - 64) return fail(DGS_ERR_ARG, "capacity_R exceeds 2^31");
        if (const int rc = setup_b(E, R, B)) return rc;
    } else {
    // (into pinned host memory: a copy to pageable memory is staged by the runtime, which held
    // the stream ~28 us past the copy before the speculative phase-B work below could start)
    htot = pinned_totals();
    if (!htot) return fail(DGS_ERR_ALLOC, "pinned host buffer allocation failed");
    herr = reinterpret_cast<uint32_t *>(htot + 8);
    DGS_TRY_HIP(hipMemcpyAsync(htot, totals, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DGS_TRY_HIP(hipMemcpyAsync(herr + 0, rs_s + plan_s.o_tickets + 63 * 4, 4, hipMemcpyDeviceToHost, s));
    DGS_TRY_HIP(hipMemcpyAsync(herr + 1, rs_h + plan_h.o_tickets + 63 * 4, 4, hipMemcpyDeviceToHost, s));
    // the one host sync (num_rendered is a Python int): on an event right after the copy, so the
    // speculative phase B enqueued behind it keeps the GPU busy while the host reads the totals
    hipEvent_t copied = nullptr;
    DGS_TRY_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    struct EventGuard {
        hipEvent_t e;
        ~EventGuard() { if (e) (void)hipEventDestroy(e); }
    } copied_guard{copied};
    DGS_TRY_HIP(hipEventRecord(copied, s));
    const SizeSpec spec = size_spec_get(P, N, D);
    if (spec.E >= 0) {
        const int rc = setup_b(spec.E + spec.E / 8 + 1024, spec.R + spec.R / 8 + 1024, B);
        if (rc) return rc;
    }
    DGS_TRY_HIP(hipEventSynchronize(copied));
    if (hipEvent_t g = giveup_copied()) DGS_TRY_HIP(hipEventSynchronize(g));  // (word 9 has landed)
    // a radix look-back gave up (dgs_radix.h; never observed): this binning's sample / home sort,
    // or the previous binning's entry sort on this thread (its word lands at the end of that call)
    if (herr[0] || herr[1] || herr[2]) {
        const bool prev = herr[2] != 0u;
        herr[0] = herr[1] = herr[2] = 0u;
        return fail(DGS_ERR_HIP, prev ? "the previous binning's entry sort failed (a radix look-back gave up): its "
                                        "results were invalid"
                                      : "binning: a radix sort's look-back gave up (sample or home sort)");
    }
    R = htot[0];
    E = htot[1];
    Es = htot[4];
    *num_rendered = R;
    if (dev_grid) {
        const int32_t *g = reinterpret_cast<const int32_t *>(htot + 2);
        for (int d = 0; d < D; ++d) {
            dev_grid[d] = g[d];
            std::memcpy(&dev_off[d], &g[2 + d], 4);
        }
    }
    if (E >= (1LL << 31) - 64) return fail(DGS_ERR_ARG, "too many fine (Gaussian, cell) entries");
    // the D = 2 sub lists live at 4 gbeg + k n in sub_ent, addressed by int32 (sub_lbeg/lmid/lend)
    if (nsub && kSubPerCell * E >= (1LL << 31) - 64)
        return fail(DGS_ERR_ARG, "too many fine (Gaussian, cell) entries for the sub-cell lists (4 E >= 2^31)");
    if (R >= (1LL << 31) - 64) return fail(DGS_ERR_ARG, "num_rendered exceeds 2^31 (32-bit tile lists)");
    size_spec_put(P, N, D, E, R);
    if (E > B.Ecap || R > B.Rcap) {  // no speculation, or this call's lists do not fit it
        const int rc = setup_b(E, R, B);
        if (rc) return rc;
    }
    }
    const Layout &L = B.L;
    const int64_t bwd_cap = B.bwd_cap;
    char *gbuf = B.gbuf;
    int32_t *counters = reinterpret_cast<int32_t *>(gbuf + L.o_counts);
    int32_t *cell_gbeg = reinterpret_cast<int32_t *>(gbuf + L.o_cell_gbeg);
    int32_t *cell_gmid = reinterpret_cast<int32_t *>(gbuf + L.o_cell_gmid);
    int32_t *cell_gend = reinterpret_cast<int32_t *>(gbuf + L.o_cell_gend);
    uint32_t *entries = reinterpret_cast<uint32_t *>(gbuf + L.o_entries);
    uint2 *bwd_units = reinterpret_cast<uint2 *>(gbuf + L.o_bwd_units);
    uint32_t *ekeys = B.ekeys, *evals = B.evals, *ekeys_sorted = B.ekeys_sorted, *svals = B.svals;
    int32_t *hbeg = B.hbeg, *hend = B.hend;
    const bool k16 = B.k16;
    const int ebits = B.ebits;

    // ---- cell lists: the sort path's entries (sorted by (cell, flag)), then per cell the
    // gathered local entries (ascending id), the sorted unflagged and the flagged ones
    // (capturable binning: Es / E are the capacities; the sort-path count on the device, esdev)
    const int64_t *esdev = capmode ? totals + 4 : nullptr;
    const uint64_t escap = capmode ? (uint64_t)Es : ~0ull;
    if (Es > 0) {
        const unsigned fb = (unsigned)((P + kFillBlock - 1) / kFillBlock);
        if (k16) {
            k_fine_fill<uint16_t><<<fb, kFillBlock, 0, s>>>(P, G, igm, igc, cell_sbeg, cell_send, cell_box, foffs,
                                                            fcount, greach, fbg, irect,
                                                            reinterpret_cast<uint16_t *>(ekeys), evals, counters, escap);
            k_wide<true, uint16_t><<<kWideBlocks, kBlock, 0, s>>>(G, igm, igc, cell_sbeg, cell_send, cell_box, fbg, wq,
                                                                  nwq, nullptr, foffs,
                                                                  reinterpret_cast<uint16_t *>(ekeys), evals, escap,
                                                                  nullptr, counters);
        } else {
            k_fine_fill<uint32_t><<<fb, kFillBlock, 0, s>>>(P, G, igm, igc, cell_sbeg, cell_send, cell_box, foffs,
                                                            fcount, greach, fbg, irect, ekeys, evals, counters, escap);
            k_wide<true, uint32_t><<<kWideBlocks, kBlock, 0, s>>>(G, igm, igc, cell_sbeg, cell_send, cell_box, fbg, wq,
                                                                  nwq, nullptr, foffs, ekeys, evals, escap, nullptr,
                                                                  counters);
        }
        DGS_LAUNCH_CHECK(s, debug);
        // (values: the entries' positions q, for the backward's slots; k_copy_sorted gathers evals[q])
        DGS_TRY_HIP(k16 ? radix_sort<uint16_t>(B.plan_e, Es, B.rs_e, reinterpret_cast<const uint16_t *>(ekeys),
                                               reinterpret_cast<uint16_t *>(ekeys_sorted), nullptr, svals, s, false,
                                               RsNone{}, esdev)
                        : radix_sort<uint32_t>(B.plan_e, Es, B.rs_e, ekeys, ekeys_sorted, nullptr, svals, s, false,
                                               RsNone{}, esdev));
        DGS_LAUNCH_CHECK(s, debug);
        if (k16)
            k_identify<uint16_t><<<grid_for(Es), kBlock, 0, s>>>(Es, reinterpret_cast<const uint16_t *>(ekeys_sorted),
                                                                 2u * (uint32_t)ncells, hbeg, hend, 1, 0u, nullptr,
                                                                 nullptr, 0, esdev);
        else
            k_identify<uint32_t><<<grid_for(Es), kBlock, 0, s>>>(Es, ekeys_sorted, 2u * (uint32_t)ncells, hbeg, hend, 1,
                                                                 0u, nullptr, nullptr, 0, esdev);
        DGS_LAUNCH_CHECK(s, debug);
    }
    {  // per cell: [gathered (ascending id) + sorted unflagged | sorted flagged] = [gbeg, gmid, gend)
        const uint32_t *c2 = cnt2;
        const int32_t *hb = hbeg, *he = hend;
        uint32_t *gc = gcnt;
        int32_t *gb_ = cell_gbeg, *gm_ = cell_gmid, *ge_ = cell_gend;
        int32_t *gs_ = reinterpret_cast<int32_t *>(gbuf + L.o_cell_gsort);  // (where each sorted part begins)
        const int64_t ecap = E;  // (exact here, or the capturable binning's capacity: lists clamped into it)
        DGS_TRY_HIP((fused_scan<1, 1>(
            (int64_t)ncells, B.fs_cells,
            [=] __device__(int64_t c, uint64_t *x) {
                uint32_t g = 0;
                for (int q = 0; q < kGatherRows; ++q) g += c2[c * kGatherRows + q];
                gc[c] = g;
                x[0] = g + (uint32_t)(he[2 * c] - hb[2 * c]) + (uint32_t)(he[2 * c + 1] - hb[2 * c + 1]);
            },
            [=] __device__(int64_t c, const uint64_t *, const uint64_t *ex) {
                const int64_t b = (int64_t)ex[0];
                const int64_t mid = b + (int64_t)gc[c] + (he[2 * c] - hb[2 * c]);
                gb_[c] = (int32_t)min(b, ecap);
                gm_[c] = (int32_t)min(mid, ecap);
                ge_[c] = (int32_t)min(mid + (he[2 * c + 1] - hb[2 * c + 1]), ecap);
                gs_[c] = (int32_t)min(b + (int64_t)gc[c], ecap);
            },
            [=] __device__(const uint64_t *) {}, s)));
        DGS_LAUNCH_CHECK(s, debug);
    }
    if (D == 2 && (capmode || E > Es)) {
        k_gather<true><<<gather_blocks, kBlock, 0, s>>>(G, P, greach, lrows, hstart, rmax, cnt2, nullptr, cell_gbeg,
                                                        entries, (uint32_t)E);
        DGS_LAUNCH_CHECK(s, debug);
    }
    if (Es > 0) {
        uint32_t *eq = reinterpret_cast<uint32_t *>(gbuf + L.o_esum_q);
        if (k16)
            k_copy_sorted<uint16_t><<<grid_for(Es), kBlock, 0, s>>>(
                Es, reinterpret_cast<const uint16_t *>(ekeys_sorted), svals, evals, hbeg, cell_gbeg, cell_gmid, gcnt,
                entries, eq, esdev, E);
        else
            k_copy_sorted<uint32_t><<<grid_for(Es), kBlock, 0, s>>>(Es, ekeys_sorted, svals, evals, hbeg, cell_gbeg,
                                                                    cell_gmid, gcnt, entries, eq, esdev, E);
        DGS_LAUNCH_CHECK(s, debug);
    }
    {  // work units: forward (cell, 64 pair-aligned samples), backward (cell, 64 list entries)
        const int32_t *sb_ = cell_sbeg, *se_ = cell_send, *gb_ = cell_gbeg, *ge_ = cell_gend;
        uint2 *fu = fwd_units, *bu = bwd_units;
        int32_t *cnt = counters;
        DGS_TRY_HIP((fused_scan<2, 1>(
            (int64_t)ncells, B.fs_units,
            [=] __device__(int64_t c, uint64_t *x) {
                const int ns = se_[c] - sb_[c], ng = ge_[c] - gb_[c];
                const int npairs = ((se_[c] + 1) >> 1) - (sb_[c] >> 1);
                x[0] = ns > 0 && ng > 0 ? (uint64_t)((npairs + kFwdUnit / 2 - 1) / (kFwdUnit / 2)) : 0u;
                x[1] = ns > 0 ? (uint64_t)((ng + kWave - 1) / kWave) : 0u;
            },
            [=] __device__(int64_t c, const uint64_t *x, const uint64_t *ex) {
                for (uint32_t b = 0; b < (uint32_t)x[0]; ++b)
                    fu[ex[0] + b] = make_uint2((uint32_t)c, (uint32_t)(sb_[c] & ~1) + b * kFwdUnit);
                for (uint32_t b = 0; b < (uint32_t)x[1]; ++b)
                    bu[ex[1] + b] = make_uint2((uint32_t)c, (uint32_t)gb_[c] + b * kWave);
            },
            [=] __device__(const uint64_t *t) {
                cnt[kNumFwdUnits] = (int32_t)t[0];
                cnt[kNumBwdUnits] = (int32_t)t[1];
            },
            s)));
        DGS_LAUNCH_CHECK(s, debug);
    }
    if (nsub) {  // the forward's sub lists and sub units (D = 2)
        const float2 *gmean = reinterpret_cast<const float2 *>(gbuf + L.o_gmean);
        const float4 *gcon = reinterpret_cast<const float4 *>(gbuf + L.o_gcon);
        int32_t *sub_lbeg = reinterpret_cast<int32_t *>(gbuf + L.o_sub_lbeg);
        int32_t *sub_lmid = reinterpret_cast<int32_t *>(gbuf + L.o_sub_lmid);
        int32_t *sub_lend = reinterpret_cast<int32_t *>(gbuf + L.o_sub_lend);
        int32_t *sub_lthin = reinterpret_cast<int32_t *>(gbuf + L.o_sub_lthin);
        uint32_t *sub_ent = reinterpret_cast<uint32_t *>(gbuf + L.o_sub_ent);
        const SubListArgs sa{ncells,   G.CT,     cell_gbeg, cell_gmid, cell_gend, entries,  gmean,  gcon,
                             cell_box, sub_box,  sub_lbeg,  sub_lmid,  sub_lend,  sub_lthin, sub_ent,
                             (float)(G.qf * (1.0 + 1e-4))};
        k_sub_lists<<<(unsigned)((ncells + kWavesPerBlock - 1) / kWavesPerBlock), kBlock, 0, s>>>(sa);
        DGS_LAUNCH_CHECK(s, debug);
        // forward sub units per sub-cell with samples and entries: (sub-cell, kSubPairs pairs)
        const int32_t *ssb = sub_sbeg, *sse = sub_send, *slb = sub_lbeg, *sle = sub_lend;
        uint2 *su = fsub_units;
        int32_t *cnt = counters;
        DGS_TRY_HIP((fused_scan<1, 1>(
            (int64_t)nsub, B.fs_sub,
            [=] __device__(int64_t k, uint64_t *x) {
                const int ns = sse[k] - ssb[k];
                const int npairs = ((sse[k] + 1) >> 1) - (ssb[k] >> 1);
                x[0] = ns > 0 && sle[k] > slb[k] ? (uint64_t)((npairs + kSubPairs - 1) / kSubPairs) : 0u;
            },
            [=] __device__(int64_t k, const uint64_t *x, const uint64_t *ex) {
                for (uint32_t b = 0; b < (uint32_t)x[0]; ++b)
                    su[ex[0] + b] = make_uint2((uint32_t)k, (uint32_t)(ssb[k] & ~1) + b * 2u * kSubPairs);
            },
            [=] __device__(const uint64_t *t) { cnt[kNumFwdSubUnits] = (int32_t)t[0]; }, s)));
        DGS_LAUNCH_CHECK(s, debug);
    }

    // ---- reference-layout ranges (uint2 per tile + 8 slack bytes, zero-filled) and the
    // call-time path's tables: per-tile list starts and unit counts (its tile lists -- the
    // reference's point_list -- are sorted at the first call that may need them: ensure_ref_lists)
    // (launched with the copies and the headers below: k_binning_tail)
    CopySpec c{};
    {  // the binned tensors as passed (each forward / backward compares its inputs with them)
        const int S3 = D * (D + 1) / 2;
        c.src[0] = reinterpret_cast<const uint32_t *>(means); c.dst[0] = reinterpret_cast<uint32_t *>(gbuf + L.o_mcopy);
        c.n[0] = (int64_t)P * D;
        c.src[1] = reinterpret_cast<const uint32_t *>(conics); c.dst[1] = reinterpret_cast<uint32_t *>(gbuf + L.o_ccopy);
        c.n[1] = (int64_t)P * S3;
        c.src[2] = reinterpret_cast<const uint32_t *>(samples); c.dst[2] = reinterpret_cast<uint32_t *>(sbuf + L0.o_scopy);
        c.n[2] = (int64_t)N * D;
        c.count = 3;
    }

    // ---- headers
    static std::atomic<uint64_t> stamp_counter{0x5eed0000ull};
    Header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = kMagic;
    h.version = kVersion;
    h.P = P; h.D = D; h.N = N; h.T = G.T;
    h.grid[0] = G.grid[0]; h.grid[1] = G.grid[1];
    h.off[0] = G.off[0]; h.off[1] = G.off[1];
    h.n = G.n; h.CT = G.CT; h.ncells = ncells;
    h.R = R; h.E = E;
    h.fwd_cap = fwd_cap; h.bwd_cap = bwd_cap;
    h.o_counts = L.o_counts; h.o_perm = L.o_perm; h.o_cell_gbeg = L.o_cell_gbeg;
    h.o_cell_gend = L.o_cell_gend; h.o_entries = L.o_entries; h.o_bwd_units = L.o_bwd_units;
    h.o_cell_gmid = L.o_cell_gmid;
    h.g_bytes = L.g_bytes;
    h.o_sorted = L0.o_sorted; h.o_cell_sbeg = L0.o_cell_sbeg; h.o_cell_send = L0.o_cell_send;
    h.o_fwd_units = L0.o_fwd_units; h.o_cell_box = L0.o_cell_box; h.s_bytes = L0.s_bytes;
    h.o_gmean = L.o_gmean; h.o_gcon = L.o_gcon; h.o_fsrows = L0.o_fsrows;
    h.o_mcopy = L.o_mcopy; h.o_ccopy = L.o_ccopy; h.o_rlist = L.o_rlist; h.o_rtab = L.o_rtab; h.o_rref = L.o_rref;
    h.o_esum_q = L.o_esum_q; h.o_cell_gsort = L.o_cell_gsort; h.o_goff = L.o_goff; h.Es = Es;
    h.o_scopy = L0.o_scopy;
    h.o_sub_sbeg = L0.o_sub_sbeg; h.o_sub_send = L0.o_sub_send; h.o_sub_box = L0.o_sub_box;
    h.o_fsub_units = L0.o_fsub_units;
    h.o_sub_lbeg = L.o_sub_lbeg; h.o_sub_lmid = L.o_sub_lmid; h.o_sub_lend = L.o_sub_lend; h.o_sub_ent = L.o_sub_ent;
    h.o_sub_lthin = L.o_sub_lthin;
    h.fsub_cap = fsub_cap_of(D, N, ncells); h.esub_cap = esub_cap_of(D, E);
    h.stamp = ++stamp_counter;
    TailSpec ts{G.T, gtile, stile, reinterpret_cast<uint2 *>(rbuf), reinterpret_cast<uint2 *>(srbuf),
                reinterpret_cast<uint32_t *>(gbuf + L.o_rtab), gbuf, sbuf};
    if (capmode) {
        ts.capture = 1;
        ts.D = D;
        ts.totals = totals;
        ts.Rcap = R; ts.Ecap = E; ts.Escap = Es;
        ts.dgrid = reuse ? nullptr : cgrid;  // (no grid check for fixed samples)
        ts.doff = reuse ? nullptr : coff;
        for (int d = 0; d < 2; ++d) { ts.grid[d] = G.grid[d]; ts.off[d] = G.off[d]; }
        ts.R_out = copt->num_rendered_device;
        ts.status = copt->status_device;
        ts.sticky = (copt->flags & DGS_BIN_STATUS_STICKY) ? 1 : 0;
    }
    k_binning_tail<<<1024, kBlock, 0, s>>>(c, ts, h);
    DGS_LAUNCH_CHECK(s, debug);

    // launch-size hint: the unit capacities (the exact counts stay on the device and the render
    // kernels grid-stride over them; surplus waves exit at once), so the binning needs no second
    // host sync.  nunsafe: the kUnsafe entry count k_fine_count read back at the sync (0: the
    // forward's unsafe-only tail pass is not launched).
    UnitHint uh;
    uh.gbuf = gbuf; uh.sbuf = sbuf; uh.gbytes = L.g_bytes; uh.sbytes = L0.s_bytes;
    // (capturable binning: the counts are the device's; unknown here -> every pass launched)
    uh.nfwd = fwd_cap; uh.nbwd = bwd_cap; uh.nunsafe = capmode ? -1 : htot[6]; uh.nthin = capmode ? -1 : htot[7];
    uh.capture = capmode;
    uh.own_grid = own_grid;
    uh.nfsub = fsub_cap_of(D, N, ncells);
    uh.ncells = ncells;
    uh.P = P; uh.D = D; uh.N = N; uh.R = R; uh.E = E; uh.Es = Es;
    uh.hdr = h;
    uh.ref_built = false;
    uh.ref_done = nullptr;
    hint_put(uh);
    if (Es > 0 && herr) {  // the entry sort's give-up word, checked at this thread's next binning sync
        DGS_TRY_HIP(hipMemcpyAsync(herr + 2, B.rs_e + B.plan_e.o_tickets + 63 * 4, 4, hipMemcpyDeviceToHost, s));
        hipEvent_t &g = giveup_copied();
        if (!g) DGS_TRY_HIP(hipEventCreateWithFlags(&g, hipEventDisableTiming));
        DGS_TRY_HIP(hipEventRecord(g, s));
    }
    return DGS_OK;
}
// Sorts the call-time path's tile lists (see ensure_ref_lists in dgs_internal.h) of the binning
// whose header is h: keys in caller-id order at the reference's scan offsets, then a stable sort
// by tile (sampler_impl.cu:265-283).  Stream-ordered scratch.
static int build_ref_lists(const Header &h, char *gbuf, hipStream_t s, int debug) {
    const int64_t R = h.R, P = h.P;
    if (R <= 0 || P <= 0) return DGS_OK;
    Geom G{};
    G.D = h.D; G.T = h.T; G.n = h.n; G.CT = h.CT; G.ncells = h.ncells;
    G.grid[0] = h.grid[0]; G.grid[1] = h.grid[1];
    G.off[0] = h.off[0]; G.off[1] = h.off[1];
    G.fs = (double)kTile / h.n;
    G.ifs = 1.0 / G.fs;
    G.qf = kQCut;  // (the tile lists make no cut)
    G.rf = 1.0;
    const int rbits = bit_length((uint64_t)(G.T > 1 ? G.T - 1 : 1));
    uint32_t *rlist = reinterpret_cast<uint32_t *>(gbuf + h.o_rlist);
    const RadixPlan plan = radix_plan(R, rbits);
    const size_t kb = align_up(4 * (size_t)R, 256);
    char *scr = nullptr;
    note_internal_alloc();  // (the call-time path's first use: dgs.h)
    DGS_TRY_HIP(hipMallocAsync(reinterpret_cast<void **>(&scr), 3 * kb + plan.bytes, s));
    uint32_t *keys = reinterpret_cast<uint32_t *>(scr), *vals = reinterpret_cast<uint32_t *>(scr + kb);
    uint32_t *keys_sorted = reinterpret_cast<uint32_t *>(scr + 2 * kb);
    hipError_t e = hipMemsetAsync(scr + 3 * kb, 0, plan.zero_bytes, s);
    if (e == hipSuccess) {
        k_ref_keys<<<grid_for(P), kBlock, 0, s>>>((int)P, R, G, reinterpret_cast<const float2 *>(gbuf + h.o_gmean),
                                                  reinterpret_cast<const int32_t *>(gbuf + h.o_perm),
                                                  reinterpret_cast<const uint32_t *>(gbuf + h.o_rref), keys, vals);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = radix_sort<uint32_t>(plan, R, scr + 3 * kb, keys, keys_sorted, vals, rlist, s);
    const hipError_t f = hipFreeAsync(scr, s);
    DGS_TRY_HIP(e);
    DGS_TRY_HIP(f);
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

static std::mutex g_ref_mu;  // one build per binning, whichever stream asks first

int ensure_ref_lists(const void *gbuf, size_t gbytes, const void *sbuf, size_t sbytes, hipStream_t s, int debug) {
    std::lock_guard<std::mutex> lk(g_ref_mu);
    UnitHint h;
    const bool known = hint_get(gbuf, gbytes, sbuf, sbytes, &h);
    if (!known || (h.capture && !h.ref_built)) {  // a foreign buffer (or a capturable binning's: R is
                                                  // on the device): its header, then a build
        Header hd;
        DGS_TRY_HIP(hipMemcpyAsync(&hd, gbuf, sizeof(hd), hipMemcpyDeviceToHost, s));
        DGS_TRY_HIP(hipStreamSynchronize(s));
        if (hd.magic != kMagic || hd.version != kVersion || hd.g_bytes > gbytes || hd.R < 0 ||
            hd.R >= (1LL << 31))
            return DGS_OK;  // (not a binning: the render kernels' own header check makes it loud)
        // A capturable binning that overflowed a capacity (or binned with a stale grid) clamped
        // its header's R and left its lists short: there is no pair set to evaluate other tensors
        // on.  The status word said so; re-bin eagerly (no out-of-bounds lists).
        if (hd.zero[0])
            return fail(DGS_ERR_BUFFER, "the binning's status is non-zero (a capacity overflowed or the grid changed): "
                                        "re-bin before calling with tensors other than the binned ones");
        return build_ref_lists(hd, static_cast<char *>(const_cast<void *>(gbuf)), s, debug);
    }
    if (h.ref_built) {
        if (h.ref_done) DGS_TRY_HIP(hipStreamWaitEvent(s, h.ref_done, 0));
        return DGS_OK;
    }
    if (int rc = build_ref_lists(h.hdr, static_cast<char *>(const_cast<void *>(gbuf)), s, debug)) return rc;
    hipEvent_t ev = nullptr;
    DGS_TRY_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (hipEventRecord(ev, s) != hipSuccess) {
        (void)hipEventDestroy(ev);
        return fail(DGS_ERR_HIP, "ensure_ref_lists: event record failed");
    }
    std::lock_guard<std::mutex> hl(g_hint_mu);
    auto it = g_hints.find(gbuf);
    if (it != g_hints.end() && it->second.hdr.stamp == h.hdr.stamp) {
        hint_drop(it->second);
        it->second.ref_built = true;
        it->second.ref_done = ev;
    } else {
        (void)hipEventDestroy(ev);  // (re-binned meanwhile)
    }
    return DGS_OK;
}
}  // namespace dgs

// Tuning hook: k_fine_count's phase cycle sums of a DGS_FC_PROF build (reset after reading).
extern "C" int dgs_debug_fc_prof(unsigned long long *out8) {
#if DGS_FC_PROF
    DGS_TRY_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(dgs::g_fc_prof), 64));
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DGS_TRY_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dgs::g_fc_prof), z, 64));
    return DGS_OK;
#else
    (void)out8;
    return dgs::fail(DGS_ERR_ARG, "not a DGS_FC_PROF build");
#endif
}

// Test hook (not on the reference API, not in include/): the binning's radix sort on its own,
// key_bytes 2 or 4, stream-ordered scratch.  tests/test_gpu_radix.py checks it against a stable
// CPU argsort.
extern "C" int dgs_test_radix_sort(int64_t n, int bits, int key_bytes, const void *kin, void *kout,
                                   const uint32_t *vin, uint32_t *vout, dgs_stream_t stream) {
    using namespace dgs;
    if (n < 0 || bits < 1 || bits > (key_bytes == 2 ? 16 : 32) || (key_bytes != 2 && key_bytes != 4))
        return fail(DGS_ERR_ARG, "dgs_test_radix_sort: bad arguments");
    if (n == 0) return DGS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const RadixPlan plan = radix_plan(n, bits);
    char *scr = nullptr;
    note_internal_alloc();
    DGS_TRY_HIP(hipMallocAsync(reinterpret_cast<void **>(&scr), plan.bytes, s));
    hipError_t e = hipMemsetAsync(scr, 0, plan.zero_bytes, s);
    if (e == hipSuccess)
        e = key_bytes == 2 ? radix_sort<uint16_t>(plan, n, scr, static_cast<const uint16_t *>(kin),
                                                  static_cast<uint16_t *>(kout), vin, vout, s)
                           : radix_sort<uint32_t>(plan, n, scr, static_cast<const uint32_t *>(kin),
                                                  static_cast<uint32_t *>(kout), vin, vout, s);
    uint32_t gave_up = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(&gave_up, scr + plan.o_tickets + 63 * 4, 4, hipMemcpyDeviceToHost, s);
    const hipError_t f = hipFreeAsync(scr, s);
    DGS_TRY_HIP(e);
    DGS_TRY_HIP(f);
    DGS_TRY_HIP(hipStreamSynchronize(s));
    if (gave_up) return fail(DGS_ERR_HIP, "dgs_test_radix_sort: a look-back gave up");
    return DGS_OK;
}

extern "C" int dgs_preprocess(int P, int D, int N, const float *means, const float *covariances,
                              const float *conics, const float *samples, const int *grid,
                              const float *grid_offset, float *radii, dgs_alloc_fn alloc,
                              void *alloc_ctx, int64_t *num_rendered, dgs_stream_t stream,
                              int debug) {
    return preprocess_body(P, D, N, means, covariances, conics, samples, grid, grid_offset, radii, alloc,
                           alloc_ctx, num_rendered, stream, debug, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int dgs_preprocess_ex(int P, int D, int N, const float *means, const float *covariances,
                                 const float *conics, const float *samples, const int *grid,
                                 const float *grid_offset, const dgs_bin_options *opts, float *radii,
                                 dgs_alloc_fn alloc, void *alloc_ctx, int64_t *num_rendered,
                                 dgs_stream_t stream, int debug) {
    if (opts && opts->struct_size != sizeof(dgs_bin_options))
        return fail(DGS_ERR_ARG, "dgs_preprocess_ex: dgs_bin_options.struct_size must be sizeof(dgs_bin_options) "
                                 "(a caller built against another dgs.h; see DGS_ABI_VERSION)");
    if (opts && (opts->flags & ~(uint32_t)(DGS_BIN_STATUS_STICKY | DGS_BIN_SAMPLES_FIXED | DGS_BIN_QCUT_REFERENCE)))
        return fail(DGS_ERR_ARG, "dgs_preprocess_ex: unknown dgs_bin_options.flags");
    const uint8_t *present = opts ? opts->present : nullptr;
    const double area = opts ? opts->sample_area : 0.0;
    if (!(area >= 0.0)) return fail(DGS_ERR_ARG, "dgs_preprocess_ex: sample_area must be >= 0");
    if (opts && opts->samples_binned && opts->capacity_E > 0 && !(opts->flags & DGS_BIN_SAMPLES_FIXED))
        return fail(DGS_ERR_ARG, "dgs_preprocess_ex: samples_binned with the capturable binning (capacity_E > 0) "
                                 "needs DGS_BIN_SAMPLES_FIXED");
    return preprocess_body(P, D, N, means, covariances, conics, samples, grid, grid_offset, radii, alloc,
                           alloc_ctx, num_rendered, stream, debug, nullptr, nullptr, nullptr, nullptr, present,
                           area, opts);
}

// The speculation of dgs_preprocess_auto, per sample set: keyed by (samples pointer, N, D), the
// grid of the last call and whether to speculate on it.  A key speculates only once a read-first
// call found the same grid as the call before it (fixed samples: every call after the second
// bins once, with no extra sync).  A miss turns it back to read-first, so a loop that resamples
// its points every step (samples.min moves, so the offset does) pays one small extra sync per
// call instead of a second binning, and samplers that alternate keep one entry each.
struct GridGuess {
    const void *key = nullptr;
    int N = 0, D = 0;
    int grid[2] = {0, 0};
    float off[2] = {0.0f, 0.0f};
    bool speculate = false;
    uint64_t used = 0;
};
static std::mutex g_grid_mu;
static GridGuess g_guess[8];
static uint64_t g_guess_tick = 0;

static GridGuess *guess_slot(const void *key, int N, int D) {  // caller holds g_grid_mu
    GridGuess *lru = &g_guess[0];
    for (GridGuess &e : g_guess) {
        if (e.key == key && e.N == N && e.D == D && e.used) return &e;
        if (e.used < lru->used) lru = &e;
    }
    *lru = GridGuess{};
    lru->key = key; lru->N = N; lru->D = D;
    return lru;
}

static bool same_grid(int D, const int *ga, const float *oa, const int *gb, const float *ob) {
    for (int d = 0; d < D; ++d)
        if (ga[d] != gb[d] || std::memcmp(&oa[d], &ob[d], 4) != 0) return false;
    return true;
}

extern "C" int64_t dgs_sample_reuse_count(void) { return g_sample_reuse.load(std::memory_order_relaxed); }

extern "C" int dgs_preprocess_auto(int P, int D, int N, const float *means, const float *covariances,
                                   const float *conics, const float *samples, float *radii,
                                   dgs_alloc_fn alloc, void *alloc_ctx, int64_t *num_rendered,
                                   int *grid_out, float *offset_out, dgs_stream_t stream, int debug) {
    return dgs_preprocess_auto_ex(P, D, N, means, covariances, conics, samples, nullptr, radii, alloc, alloc_ctx,
                                  num_rendered, grid_out, offset_out, stream, debug);
}

extern "C" int dgs_preprocess_auto_ex(int P, int D, int N, const float *means, const float *covariances,
                                      const float *conics, const float *samples, const dgs_bin_options *opts,
                                      float *radii, dgs_alloc_fn alloc, void *alloc_ctx, int64_t *num_rendered,
                                      int *grid_out, float *offset_out, dgs_stream_t stream, int debug) {
    if (D != 1 && D != 2) return fail(DGS_ERR_ARG, "only D = 1 or D = 2 is supported (the reference leaves D = 3 undefined)");
    if (P < 0 || N < 0 || !alloc || !num_rendered || !grid_out || !offset_out)
        return fail(DGS_ERR_ARG, "dgs_preprocess_auto: bad arguments");
    if (opts && opts->struct_size != sizeof(dgs_bin_options))
        return fail(DGS_ERR_ARG, "dgs_preprocess_auto_ex: dgs_bin_options.struct_size must be sizeof(dgs_bin_options) "
                                 "(a caller built against another dgs.h; see DGS_ABI_VERSION)");
    if (opts && ((opts->flags & ~(uint32_t)DGS_BIN_QCUT_REFERENCE) || opts->capacity_E > 0))
        return fail(DGS_ERR_ARG, "dgs_preprocess_auto_ex: flags and capacities are for dgs_preprocess_ex");
    const uint8_t *present = opts ? opts->present : nullptr;
    const double area = opts ? opts->sample_area : 0.0;
    if (!(area >= 0.0)) return fail(DGS_ERR_ARG, "dgs_preprocess_auto_ex: sample_area must be >= 0");
    *num_rendered = 0;
    if (P == 0 || N == 0) return DGS_OK;  // sample_points.cu:69: nothing to bin
    {  // the same samples, binned earlier on their own grid: that grid (no grid pass, no speculation)
        UnitHint ph;
        if (opts && opts->samples_binned && hint_by_sbuf(opts->samples_binned, opts->samples_binned_bytes, &ph) &&
            ph.own_grid && ph.hdr.N == N && ph.hdr.D == D) {
            const int g[2] = {ph.hdr.grid[0], ph.hdr.grid[1]};
            const float o[2] = {ph.hdr.off[0], ph.hdr.off[1]};
            for (int d = 0; d < D; ++d) { grid_out[d] = g[d]; offset_out[d] = o[d]; }
            return preprocess_body(P, D, N, means, covariances, conics, samples, g, o, radii, alloc, alloc_ctx,
                                   num_rendered, stream, debug, nullptr, nullptr, nullptr, nullptr, present, area, opts,
                                   true);
        }
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // sample_points.cu:70-74 on the device (torch's CUDA arithmetic, k_bounds_final)
    const int nparts = (int)std::min<int64_t>(1024, grid_for(N));
    const size_t pbytes = align_up(sizeof(float) * 4 * nparts, 256);
    float *part = static_cast<float *>(alloc(alloc_ctx, DGS_BUF_SCRATCH, pbytes + 256));
    if (!part) return fail(DGS_ERR_ALLOC, "scratch allocation failed");
    char *gb = reinterpret_cast<char *>(part) + pbytes;
    int *dgrid = reinterpret_cast<int *>(gb);
    float *doff = reinterpret_cast<float *>(gb + 16);
    k_bounds_partial<<<nparts, kBlock, 0, s>>>(N, D, samples, part);
    k_bounds_final<<<1, kBlock, 0, s>>>(nparts, D, part, dgrid, doff);
    DGS_LAUNCH_CHECK(s, debug);
    int guess[2] = {1, 1}, prev[2] = {0, 0};
    float goff[2] = {0.0f, 0.0f}, poff[2] = {0.0f, 0.0f};
    bool speculate, had;
    {
        std::lock_guard<std::mutex> lk(g_grid_mu);
        GridGuess *e = guess_slot(samples, N, D);
        had = e->used != 0;
        speculate = had && e->speculate;
        for (int d = 0; d < D; ++d) { prev[d] = guess[d] = e->grid[d]; poff[d] = goff[d] = e->off[d]; }
        e->used = ++g_guess_tick;
    }
    if (!speculate) {  // read-first: one small extra sync, then one binning
        DGS_TRY_HIP(hipMemcpyAsync(guess, dgrid, sizeof(int) * D, hipMemcpyDeviceToHost, s));
        DGS_TRY_HIP(hipMemcpyAsync(goff, doff, sizeof(float) * D, hipMemcpyDeviceToHost, s));
        DGS_TRY_HIP(hipStreamSynchronize(s));
    }
    // Bin with the guess; the device grid comes back with the totals at the body's one sync.  A
    // wrong guess bins consistently (sample keys clamp, tile ids wrap), so it is only redone.
    int dg[2] = {0, 0};
    float dof[2] = {0.0f, 0.0f};
    int rc = preprocess_body(P, D, N, means, covariances, conics, samples, guess, goff, radii, alloc, alloc_ctx,
                             num_rendered, stream, debug, dgrid, doff, dg, dof, present, area, opts, true);
    if (rc) return rc;
    const bool hit = same_grid(D, dg, dof, guess, goff);
    {
        std::lock_guard<std::mutex> lk(g_grid_mu);
        GridGuess *e = guess_slot(samples, N, D);
        e->speculate = speculate ? hit : (had && same_grid(D, dg, dof, prev, poff));
        for (int d = 0; d < D; ++d) { e->grid[d] = dg[d]; e->off[d] = dof[d]; }
        e->used = ++g_guess_tick;
    }
    if (!hit)
        rc = preprocess_body(P, D, N, means, covariances, conics, samples, dg, dof, radii, alloc, alloc_ctx,
                             num_rendered, stream, debug, nullptr, nullptr, nullptr, nullptr, present, area, opts, true);
    for (int d = 0; d < D; ++d) { grid_out[d] = dg[d]; offset_out[d] = dof[d]; }
    return rc;
}


extern "C" int dgs_binning_info(const void *binning, size_t binning_bytes, const void *sample_binning,
                                size_t sample_binning_bytes, int64_t *out) {
    UnitHint h;
    if (!out) return fail(DGS_ERR_ARG, "dgs_binning_info: out required");
    if (!hint_get(binning, binning_bytes, sample_binning, sample_binning_bytes, &h))
        return fail(DGS_ERR_BUFFER, "dgs_binning_info: buffers not binned by this process");
    out[0] = h.R;
    out[1] = h.E;
    out[2] = h.nunsafe;
    out[3] = h.ncells;
    out[4] = h.nthin;
    out[5] = h.Es;
    return DGS_OK;
}

extern "C" int dgs_exchange_sets(int P, int D, const float *means, const float *conics, int W,
                                 const double *extents, uint32_t *mask_out, int32_t *owner_out,
                                 dgs_stream_t stream) {
    if (P < 0 || (D != 1 && D != 2) || W < 1 || W > kMaxXchgRanks || !extents)
        return fail(DGS_ERR_ARG, "dgs_exchange_sets: bad arguments (1 <= W <= 32)");
    if (P == 0) return DGS_OK;
    XchgRanks R;
    R.W = W;
    for (int r = 0; r < W; ++r) { R.lo[r] = extents[2 * r]; R.hi[r] = extents[2 * r + 1]; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    k_xchg_sets<<<grid_for(P), kBlock, 0, s>>>(P, D, means, conics, R, mask_out, owner_out);
    DGS_TRY_HIP(hipGetLastError());
    return DGS_OK;
}

// ------------------------------------------------------------------------- warm-up
// A no-op launch: the first launch of any kernel of this translation unit loads its code object
// (rocprim's kernels included) onto the device; dgs_warmup does it for every unit up front.
__global__ void k_warm_preprocess() {}
namespace dgs {
hipError_t warm_preprocess(hipStream_t s) {
    k_warm_preprocess<<<1, 1, 0, s>>>();
    return hipGetLastError();
}
}  // namespace dgs
