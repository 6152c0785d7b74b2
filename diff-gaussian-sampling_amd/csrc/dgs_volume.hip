// dgs_volume.hip -- D = 3 Gaussian fields (include/dgs_volume.h).
//
// The reference has no D = 3 path (its device functions stop at D = 2, forward.cu:164-275), so
// this one carries its per-pair arithmetic to three dimensions and sums over every Gaussian
// whose contribution is not exactly 0 in fp32.  Design:
//   * one uniform grid of cells over the bounding box of the samples and the small Gaussians'
//     means, each cell at least the largest exact-zero cut half-width E_d = sqrt(210 Sigma_dd)
//     (at most 128 cells per axis); Gaussians and samples radix-sorted by cell;
//   * "small" Gaussians (well-conditioned positive-definite conic, every E_d <= 0.45) meet a
//     sample only through the torus images of the cut: per axis the displacement x = m - s
//     lies in [-E, E] (image k = 0), [2k - E, 2k] (k > 0) or [2k, 2k + E] (k < 0), the sets
//     the reference's wrap (forward.cu:149-157) maps into [-E, E].  A candidate is kept under
//     image k only if |x - 2k| <= its own cut half-width r (< 0.45): these boxes are disjoint
//     over k, so no pair is evaluated twice even when the windows' cell ranges overlap, and
//     every pair with a non-zero contribution has |wrap(x)| = |x - 2k| <= r for its own image k.
//     (A pair kept under an image that is not its own has |wrap(x)| > 1.5: G is exactly 0.
//     pair_eval always applies the reference's wrap, so its value never depends on the window.)
//   * an axis may be open instead (dgs_volume_preprocess_axes; Hdr::open, DESIGN.md 4.8, "Open
//     axes"): the walks visit its direct image only, whose cut box test is already the one on the
//     raw distance (and inside a cut box the wrap is the identity), and the loops over the big
//     Gaussians leave its X_d unwrapped (pair_eval with Axes); nothing else knows about it;
//   * "big" Gaussians (everything else) sit in one extra cell and meet every sample;
//   * forward: lane = sample (in cell order), outputs summed in registers, no atomics;
//     backward: lane = Gaussian (in cell order) walking the samples of its images, gradients
//     in registers, no atomics; big Gaussians: one block each over every sample;
//   * gradient of the samples (k_vol_sgrad_m<MASK>, k_vol_sgrad<FN, CB>): the
//     forward's walk, lane = sample with its dL rows in registers, three sums per lane, no atomics;
//   * the forward's loop nest is written once (walk_candidates) and called with two callables by
//     k_vol_forward<FN, CB> at C > 1 and k_vol_forward_m<MASK> at C = 1, where a single function
//     is the single-bit mask; the backward kernels (k_vol_backward<FN, CB>, k_vol_backward_m<MASK>
//     for two or more functions) each hold the lane = Gaussian nest: their pair arithmetic is
//     contracted by the compiler, and its last bits move when the nest does.
//   * several functions of a field of 2..4 channels: the _mc kernels ("mask, channels", below the
//     sample gradients), one walk for every function and channel in the forward, the backward
//     (moment form, its own loop nest walk_samples) and the sample gradient.
//   * a fifth function, the trace of the laplacian (code 4, bit 4 of a mask, one component per
//     channel; the dgs_volume_*_ops entries): new instantiations of the same templates, alone at any
//     C and fused with functions 0, 1, 3 up to C = 4 ("Trace Laplacian").
//   * a sixth function, a constant-coefficient linear operator c0 u + b.grad u + W:hess u (code 5,
//     bit 5, one component per channel; the dgs_volume_*_linop entries): again new instantiations,
//     alone at any C and fused with functions 0, 1 up to C = 4.  Its ten coefficients are a trailing
//     by-value kernel argument (VCoef) that only these instantiations have ("Linear
//     operator").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>

#include "dgs.h"
#include "dgs_internal.h"
#include "dgs_scan.h"
#include "dgs_volume.h"

namespace dgs {
namespace vol {

constexpr uint32_t kVolMagic = 0x33564744u;  // "DGV3"
constexpr int kAxisCells = 128;
constexpr float kMaxReach = 0.45f;
constexpr double kVolCut = 210.0;      // X^T A X above this: power < -105, expf(power) == +0
constexpr double kVolCond = 1.0e4;     // bound on ||A||_F^3 / det A for the cut to hold in fp32

struct Hdr {
    uint32_t magic;
    int P, N, nsmall, nbig, ncells;
    int n[3];
    float lo[3], cs[3], E[3];
    float split;     // small Gaussians with every cut half-width <= split: class 0, else class 1
    float Ec[2][3];  // per class, the largest cut half-width per axis (the window reach)
    // bit d: axis d is open (dgs_volume_preprocess_axes): X_d is not wrapped and only the direct
    // image exists.  The open mask and not the periodic one, so that 0 is the all-periodic torus.
    // (In the four bytes that padded the offsets: the header, which k_vol_backward copies, keeps its size.)
    int open;
    int64_t o_gext, o_gids, o_sids, o_gstart, o_sstart, o_gpk, o_gek;
    int64_t o_mcopy, o_ccopy, o_scopy, o_flag;  // the binned tensors; flag = they differ from the call's
};
constexpr size_t kHdrBytes = 256;
static_assert(sizeof(Hdr) <= kHdrBytes, "volume header too large");
static_assert(sizeof(Hdr) == 192, "Hdr::open belongs in the padding before the offsets");
// What the kernels read of the axes, as data behind the header (Hdr keeps its size: k_vol_backward
// copies it): no kernel tests Hdr::open.  The image ranges of an axis are derived from the grid's
// extent [ilo, ihi] (image_range); an open axis has the empty extent [+inf, -inf], from which no
// image but the direct one can be reached, so the walks skip its images with the arithmetic they
// had.  lim: the wrap's limit for the pairs of the big Gaussians (Axes).
struct HdrAx {
    float ilo[3], ihi[3], lim[3];
};
static_assert(sizeof(Hdr) + sizeof(HdrAx) <= kHdrBytes, "volume header too large");

static inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// packed conic index of the symmetric entry (i, j): [c00 c01 c02 c11 c12 c22]
__host__ __device__ constexpr int pidx(int i, int j) {
    return i <= j ? i * 3 - i * (i - 1) / 2 + (j - i) : j * 3 - j * (j - 1) / 2 + (i - j);
}
// unique (sorted) index of a symmetric 3-index component i <= j <= k, in lexicographic order
__host__ __device__ constexpr int uidx3s(int i, int j, int k) {
    int n = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b)
            for (int c = b; c < 3; ++c) {
                if (a == i && b == j && c == k) return n;
                ++n;
            }
    return -1;
}
__host__ __device__ constexpr int sort3_idx(int i, int j, int k) {
    const int a = i < j ? i : j, b = i < j ? j : i;  // a <= b
    const int lo = k < a ? k : a;
    const int hi = k > b ? k : b;
    const int mid = i + j + k - lo - hi;
    return uidx3s(lo, mid, hi);
}

// Function masks (bit f = function f).  The unique (symmetric) components of a mask's functions:
// 1, 3, 6 and 10 of the 1, 3, 9 and 27 full ones; every other count derives from this one.
// Function 4 (bit 4) is the trace of the laplacian, one component ("Trace
// Laplacian"); it comes last in a concatenated row and never shares a mask with the laplacian.
__host__ __device__ constexpr int mask_ku(int mask) {
    return (mask & 1 ? 1 : 0) + (mask & 2 ? 3 : 0) + (mask & 4 ? 6 : 0) + (mask & 8 ? 10 : 0) + (mask & 16 ? 1 : 0) +
           (mask & 32 ? 1 : 0);
}
// offset of function f's unique components in a concatenated row of the mask's functions
__host__ __device__ constexpr int mask_off(int mask, int f) { return mask_ku(mask & ((1 << f) - 1)); }
// the order of the mask's highest function (the trace is of order 2: vol_mom_add<TOP>)
__host__ __device__ constexpr int mask_top(int mask) { return mask & 8 ? 3 : mask & (4 | 16 | 32) ? 2 : mask & 2 ? 1 : 0; }
constexpr int kFnTrace = DGS_VOLUME_FN_LAPLACIAN_TRACE;
// Function 5 (bit 5) is the linear operator, one component like the trace ("Linear
// operator"); it comes last in a row and shares a mask only with the gaussian and the derivative.
constexpr int kFnOp = DGS_VOLUME_FN_OPERATOR;
// The kernels' pointer structs (VOuts, VDLs) have one slot per function code 0..3; the trace and the
// operator take the laplacian's, which a mask with either never uses.
__host__ __device__ constexpr int fn_slot(int fn) { return fn == kFnTrace || fn == kFnOp ? 2 : fn; }

// The operator's coefficients as the kernels take them, by value (wave-uniform: scalar registers):
// k = [c0, b0, b1, b2, w00, 2 w01, 2 w02, w11, 2 w12, w22], the doubling done on the host (exact).
// Only the instantiations with the operator have this argument (the kernels' trailing pack CF is
// empty for every other one, so their argument lists are what they were).
struct VCoef {
    float k[10];
};
__device__ __forceinline__ const float *coef_of() { return nullptr; }
__device__ __forceinline__ const float *coef_of(const VCoef &cf) { return cf.k; }
// The operator's per-pair factor t (include/dgs_volume.h: the order of the roundings), from the
// packed conic c; half: 0.5 where c holds the off-diagonals doubled (c2 of the moment form; exact).
__device__ __forceinline__ float op_t(const float *a, const float *c, const float *k, float half = 1.0f) {
    DGS_NO_CONTRACT
    const float lin = k[1] * a[0] + k[2] * a[1] + k[3] * a[2];
    const float q = k[4] * (a[0] * a[0] - c[0]) + k[5] * (a[0] * a[1] - half * c[1]) +
                    k[6] * (a[0] * a[2] - half * c[2]) + k[7] * (a[1] * a[1] - c[3]) +
                    k[8] * (a[1] * a[2] - half * c[4]) + k[9] * (a[2] * a[2] - c[5]);
    return (k[0] + lin) + q;
}
// g = d(h t)/da = h (b + 2 W a) and e = d(h t)/dc = -h k_u (packed)
__device__ __forceinline__ void op_ge(float h, const float *a, const float *k, float *g, float *e) {
    g[0] = h * (k[1] + (2.0f * k[4] * a[0] + k[5] * a[1] + k[6] * a[2]));
    g[1] = h * (k[2] + (k[5] * a[0] + 2.0f * k[7] * a[1] + k[8] * a[2]));
    g[2] = h * (k[3] + (k[6] * a[0] + k[8] * a[1] + 2.0f * k[9] * a[2]));
    for (int q = 0; q < 6; ++q) e[q] = -h * k[4 + q];
}

template <int FN>
struct VTr {
    static constexpr int KU = mask_ku(1 << FN), K = FN == 0 || FN == kFnTrace || FN == kFnOp ? 1 : FN == 1 ? 3 : FN == 2 ? 9 : 27;
};

// unique component of the full output index f (row-major over the 3^FN indices)
template <int FN>
__host__ __device__ constexpr int umap(int f) {
    if (FN == 0 || FN == kFnTrace || FN == kFnOp) return 0;
    if (FN == 1) return f;
    if (FN == 2) return pidx(f / 3, f % 3);
    return sort3_idx(f / 9, (f / 3) % 3, f % 3);
}
// the index triple of unique component u (FN = 2: pair (i, j) = first two)
__host__ __device__ constexpr int u2i(int u, int w) {
    return w == 0 ? (u < 3 ? 0 : u < 5 ? 1 : 2) : (u < 3 ? u : u < 5 ? u - 2 : 2);
}
__host__ __device__ constexpr int u3i(int u, int w) {
    int n = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b)
            for (int c = b; c < 3; ++c) {
                if (n == u) return w == 0 ? a : w == 1 ? b : c;
                ++n;
            }
    return 0;
}

// The axes a pair is evaluated under.  Torus: every axis wraps (forward.cu:149-157), the parent's
// arithmetic with nothing added; it serves every pair of the walks, on open axes too, because a
// walk visits only the direct image of an open axis and keeps a pair only inside its cut box,
// |m - s| <= r + 1e-5 with r <= kMaxReach < 1, where the wrap is the identity.  Axes: the binning's
// Hdr::open, for the pairs of the big Gaussians, which meet every sample at any distance: an open
// axis is not wrapped.  So the hot loops of the walks hold no register for the axes: their kernels
// already take every scalar register there is, and one more live scalar costs a lane read per use.
struct Torus {};
struct Axes {
    float lim[3];  // |x| above it wraps: 1 on a periodic axis, +inf on an open one (HdrAx::lim)
};
__device__ __forceinline__ float wrap_axis(const Torus &, int, float x) {
    if (fabsf(x) > 1.0f) x = x >= 0.0f ? fmodf(x, 2.0f) - 2.0f : fmodf(x, 2.0f) + 2.0f;
    return x;
}
__device__ __forceinline__ float wrap_axis(const Axes &ax, int d, float x) {
    if (fabsf(x) > ax.lim[d]) x = x >= 0.0f ? fmodf(x, 2.0f) - 2.0f : fmodf(x, 2.0f) + 2.0f;
    return x;
}
// One pair: wrapped X (open axes: not wrapped), power (exact operation order of
// include/dgs_volume.h, no contraction, so that the numpy oracle reproduces it bit for bit), G and
// a = A X.  False: power > 0 (the reference's skip) or G == +0 (the pair adds exactly nothing; half
// of the cut box's pairs).
template <class AX>
__device__ __forceinline__ bool pair_eval(const AX &ax, const float *m, const float *s, const float *c, float *X,
                                          float &G, float *a) {
    DGS_NO_CONTRACT
    for (int d = 0; d < 3; ++d) X[d] = wrap_axis(ax, d, m[d] - s[d]);
    const float qd = c[0] * X[0] * X[0] + c[3] * X[1] * X[1] + c[5] * X[2] * X[2];
    const float qo = c[1] * X[0] * X[1] + c[2] * X[0] * X[2] + c[4] * X[1] * X[2];
    const float power = -0.5f * qd - qo;
    if (power > 0.0f) return false;
    G = expf(power);
    if (G == 0.0f) return false;  // exactly 0: adds nothing (finite values and terms)
    a[0] = c[0] * X[0] + c[1] * X[1] + c[2] * X[2];
    a[1] = c[1] * X[0] + c[3] * X[1] + c[4] * X[2];
    a[2] = c[2] * X[0] + c[4] * X[1] + c[5] * X[2];
    return true;
}

template <int FN>
__device__ __forceinline__ void terms(const float *a, const float *c, float *t, const float *cf = nullptr) {
    DGS_NO_CONTRACT
    if constexpr (FN == 0) {
        t[0] = 1.0f;
    } else if constexpr (FN == 1) {
        for (int i = 0; i < 3; ++i) t[i] = a[i];
    } else if constexpr (FN == 2) {
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int i = u2i(u, 0), j = u2i(u, 1);
            t[u] = a[i] * a[j] - c[pidx(i, j)];
        }
    } else if constexpr (FN == kFnTrace) {
        t[0] = (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) - (c[0] + c[3] + c[5]);
    } else if constexpr (FN == kFnOp) {
        t[0] = op_t(a, c, cf);
    } else {
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const int i = u3i(u, 0), j = u3i(u, 1), k = u3i(u, 2);
            t[u] = c[pidx(i, j)] * a[k] + c[pidx(i, k)] * a[j] + c[pidx(j, k)] * a[i] - a[i] * a[j] * a[k];
        }
    }
}

// g = d phi / d a and e = d phi / d c (explicit, packed conic) for phi = sum_u h_u t_u.
template <int FN>
__device__ __forceinline__ void phi_grads(const float *h, const float *a, const float *c, float *g, float *e,
                                          const float *cf = nullptr) {
    for (int i = 0; i < 3; ++i) g[i] = 0.0f;
    for (int q = 0; q < 6; ++q) e[q] = 0.0f;
    if constexpr (FN == 1) {
        for (int i = 0; i < 3; ++i) g[i] = h[i];
    } else if constexpr (FN == 2) {
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int i = u2i(u, 0), j = u2i(u, 1);
            g[i] += h[u] * a[j];
            g[j] += h[u] * a[i];
            e[pidx(i, j)] -= h[u];
        }
    } else if constexpr (FN == 3) {
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const int i = u3i(u, 0), j = u3i(u, 1), k = u3i(u, 2);
            g[k] += h[u] * c[pidx(i, j)];
            g[j] += h[u] * c[pidx(i, k)];
            g[i] += h[u] * c[pidx(j, k)];
            g[i] -= h[u] * a[j] * a[k];
            g[j] -= h[u] * a[i] * a[k];
            g[k] -= h[u] * a[i] * a[j];
            e[pidx(i, j)] += h[u] * a[k];
            e[pidx(i, k)] += h[u] * a[j];
            e[pidx(j, k)] += h[u] * a[i];
        }
    } else if constexpr (FN == kFnTrace) {
        for (int i = 0; i < 3; ++i) g[i] = 2.0f * h[0] * a[i];
        e[0] = e[3] = e[5] = -h[0];
    } else if constexpr (FN == kFnOp) {
        op_ge(h[0], a, cf, g, e);
    }
}

// Adds one pair's gradients: dX (= d/d mean) and d/d conic (packed), for loss G * phi.
__device__ __forceinline__ void pair_grads(float G, float phi, const float *X, const float *a, const float *c,
                                           const float *g, const float *e, float *dm, float *dc) {
    for (int m = 0; m < 3; ++m) {
        float Ag = 0.0f;
        for (int i = 0; i < 3; ++i) Ag += c[pidx(i, m)] * g[i];
        dm[m] += G * (Ag - a[m] * phi);
    }
    for (int p = 0; p < 3; ++p)
        for (int q = p; q < 3; ++q) {
            const float dpow = p == q ? -0.5f * X[p] * X[p] : -X[p] * X[q];
            const float da = p == q ? g[p] * X[p] : g[p] * X[q] + g[q] * X[p];
            dc[pidx(p, q)] += G * (phi * dpow + da + e[pidx(p, q)]);
        }
}

__device__ __forceinline__ int cell_axis(const Hdr &h, int d, float x) {
    const int c = (int)floorf((x - h.lo[d]) / h.cs[d]);
    return min(max(c, 0), h.n[d] - 1);
}

// Image windows of one axis for a point p and reach r: image k covers p + [xa(k), xb(k)] with
// xa/xb the displacement window (target - p).  sign = +1: targets are means (x = target - p is
// -(m - s): used with the sample as p); the windows are written for the x = m - s convention
// through `flip`.
struct Win {
    int k0, k1;  // image range
};
// range of images k whose window can reach [lo, hi] (target coordinates)
__device__ __forceinline__ Win image_range(float p, float r, float lo, float hi, bool target_is_mean) {
    // target = p + x (means, x = m - s with p = s) or p - x (samples, p = m)
    // image k >= 1 window in x: [2k - r, 2k]; k <= -1: [2k, 2k + r]
    const float tlo = target_is_mean ? lo - p : p - hi;  // x range the targets allow
    const float thi = target_is_mean ? hi - p : p - lo;
    Win w;
    w.k1 = thi >= 2.0f - r ? (int)floorf((thi + r) * 0.5f) : 0;
    w.k0 = tlo <= -2.0f + r ? -(int)floorf((r - tlo) * 0.5f) : 0;
    return w;
}
// x window of image k (x = m - s), widened by a rounding margin
__device__ __forceinline__ void image_window(int k, float r, float &xa, float &xb) {
    const float tol = 1e-5f;
    if (k == 0) { xa = -r - tol; xb = r + tol; }
    else if (k > 0) { xa = 2.0f * k - r - tol; xb = 2.0f * k + tol; }
    else { xa = 2.0f * k - tol; xb = 2.0f * k + r + tol; }
}

__device__ __forceinline__ const Hdr &hdr_of(const char *buf) { return *reinterpret_cast<const Hdr *>(buf); }
__device__ __forceinline__ const HdrAx &hax_of(const char *buf) { return *reinterpret_cast<const HdrAx *>(buf + sizeof(Hdr)); }
// The wrap limits, read where the loops over the big Gaussians start (a volatile read: a plain one
// is hoisted out of the loop over the cells and the three values then live through the walks, whose
// kernels have no scalar register to spare).
__device__ __forceinline__ Axes axes_of(const char *buf) {
    const volatile int *l = reinterpret_cast<const volatile int *>(hax_of(buf).lim);
    const auto uni = [](int bits) { return __int_as_float(__builtin_amdgcn_readfirstlane(bits)); };  // (wave-uniform)
    return {{uni(l[0]), uni(l[1]), uni(l[2])}};
}

// ------------------------------------------------------------------------------ preprocess
struct Red {
    float mlo[3], mhi[3], slo[3], shi[3], E[3];
    int nbig, pad[3];
};

__global__ void k_vol_init(Red *r) {
    if (threadIdx.x == 0) {
        for (int d = 0; d < 3; ++d) {
            r->mlo[d] = r->slo[d] = INFINITY;
            r->mhi[d] = r->shi[d] = -INFINITY;
            r->E[d] = 0.0f;
        }
        r->nbig = 0;
    }
}

__device__ __forceinline__ void atomic_min_f(float *p, float v) {
    if (!(v == v)) return;
    int *ip = reinterpret_cast<int *>(p);
    int old = *ip;
    while (v < __int_as_float(old)) {
        const int prev = atomicCAS(ip, old, __float_as_int(v));
        if (prev == old) break;
        old = prev;
    }
}
__device__ __forceinline__ void atomic_max_f(float *p, float v) {
    if (!(v == v)) return;
    int *ip = reinterpret_cast<int *>(p);
    int old = *ip;
    while (v > __int_as_float(old)) {
        const int prev = atomicCAS(ip, old, __float_as_int(v));
        if (prev == old) break;
        old = prev;
    }
}
__device__ __forceinline__ float wave_min(float v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Per Gaussian: the exact-zero cut half-widths E_d = sqrt(210 Sigma_dd) (fp64 from the conic)
// and whether the Gaussian is small (gext.w = 1); bounds of the small means, the largest E,
// the big count.
__global__ __launch_bounds__(kBlock) void k_vol_classify(int P, const float *__restrict__ means,
                                                         const float *__restrict__ conics,
                                                         float4 *__restrict__ gext, Red *__restrict__ red) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float E[3] = {0.0f, 0.0f, 0.0f};
    int big = 0;
    if (i < P) {
        double c[6], m[3];
        for (int q = 0; q < 6; ++q) c[q] = conics[(int64_t)i * 6 + q];
        for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)i * 3 + d];
        const double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
        const double m01 = a00 * a11 - a01 * a01;
        const double det = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02) + a02 * (a01 * a12 - a11 * a02);
        double fro = 0.0;
        for (int q = 0; q < 6; ++q) fro += (q == 0 || q == 3 || q == 5 ? 1.0 : 2.0) * c[q] * c[q];
        fro = sqrt(fro);
        bool small = a00 > 0.0 && m01 > 0.0 && det > 0.0 && isfinite(det) && fro * fro * fro < kVolCond * det;
        float e[3] = {0.0f, 0.0f, 0.0f};
        if (small) {
            const double s00 = (a11 * a22 - a12 * a12) / det, s11 = (a00 * a22 - a02 * a02) / det,
                         s22 = m01 / det;
            const double sd[3] = {s00, s11, s22};
            for (int d = 0; d < 3; ++d) {
                const double ed = sqrt(kVolCut * (1.0 + 1e-6) * sd[d]) * (1.0 + 1e-6) + 1e-7;
                e[d] = (float)ed;
                small = small && sd[d] > 0.0 && ed <= (double)kMaxReach && isfinite(m[d]);
            }
        }
        gext[i] = make_float4(e[0], e[1], e[2], small ? 1.0f : 0.0f);
        if (small) {
            for (int d = 0; d < 3; ++d) {
                lo[d] = hi[d] = (float)m[d];
                E[d] = e[d];
            }
        } else {
            big = 1;
        }
    }
    for (int d = 0; d < 3; ++d) {
        lo[d] = wave_min(lo[d]);
        hi[d] = wave_max(hi[d]);
        E[d] = wave_max(E[d]);
    }
    for (int o = kWave / 2; o > 0; o >>= 1) big += __shfl_xor(big, o);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        for (int d = 0; d < 3; ++d) {
            atomic_min_f(&red->mlo[d], lo[d]);
            atomic_max_f(&red->mhi[d], hi[d]);
            atomic_max_f(&red->E[d], E[d]);
        }
        if (big) atomicAdd(&red->nbig, big);
    }
}

__global__ __launch_bounds__(kBlock) void k_vol_sbounds(int N, const float *__restrict__ samples, Red *__restrict__ red) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += (int64_t)gridDim.x * kBlock)
        for (int d = 0; d < 3; ++d) {
            const float v = samples[j * 3 + d];
            lo[d] = fminf(lo[d], v);
            hi[d] = fmaxf(hi[d], v);
        }
    for (int d = 0; d < 3; ++d) {
        lo[d] = wave_min(lo[d]);
        hi[d] = wave_max(hi[d]);
    }
    if ((threadIdx.x & (kWave - 1)) == 0)
        for (int d = 0; d < 3; ++d) {
            atomic_min_f(&red->slo[d], lo[d]);
            atomic_max_f(&red->shi[d], hi[d]);
        }
}

// cell keys and the identity values.  Gaussians: class * ncells + cell (class 1: some cut
// half-width above split), big ones 2 * ncells; samples: the cell.
__global__ __launch_bounds__(kBlock) void k_vol_keys(int n, Hdr h, const float *__restrict__ pts,
                                                     const float4 *__restrict__ gext, uint32_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t key = (uint32_t)(2 * h.ncells);  // (Gaussians: class-major cells, then the big ones)
    if (!gext || gext[i].w != 0.0f) {
        int c[3];
        for (int d = 0; d < 3; ++d) {
            const float x = pts[(int64_t)i * 3 + d];
            c[d] = x == x ? cell_axis(h, d, x) : 0;
        }
        key = (uint32_t)((c[2] * h.n[1] + c[1]) * h.n[0] + c[0]);
        if (gext) {
            const float4 e = gext[i];
            if (fmaxf(fmaxf(e.x, e.y), e.z) > h.split) key += (uint32_t)h.ncells;
        }
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// start[c] = first sorted position with key >= c, for c in [0, ncells + 1]; start[ncells + 1] = n
__global__ __launch_bounds__(kBlock) void k_vol_starts(int n, int ncells, const uint32_t *__restrict__ keys,
                                                       int32_t *__restrict__ start) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (n == 0) {
        for (int c = i; c <= ncells + 1; c += gridDim.x * kBlock) start[c] = 0;
        return;
    }
    if (i >= n) return;
    const int kprev = i == 0 ? -1 : (int)keys[i - 1];
    const int k = (int)keys[i];
    for (int c = kprev + 1; c <= k; ++c) start[c] = i;
    if (i == n - 1)
        for (int c = k + 1; c <= ncells + 1; ++c) start[c] = n;
}

// Cell-sorted copies of the small Gaussians' means (id in .w) and cut half-widths: the
// forward's candidate scan reads them contiguously and rejects a candidate outside its own cut
// box before touching its conic.
__global__ __launch_bounds__(kBlock) void k_vol_pack(int nsmall, const int32_t *__restrict__ gids,
                                                     const float *__restrict__ means,
                                                     const float4 *__restrict__ gext, float4 *__restrict__ gpk,
                                                     float4 *__restrict__ gek) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nsmall) return;
    const int g = gids[i];
    gpk[i] = make_float4(means[(int64_t)g * 3], means[(int64_t)g * 3 + 1], means[(int64_t)g * 3 + 2], __int_as_float(g));
    gek[i] = gext[g];
}

// Every forward / backward compares its means, conics and samples bitwise with the binned ones:
// the cells and the packed means come from preprocess, so other tensors (an in-place optimizer
// step, moved samples) would mix old and new parameters.  On a difference the call writes NaN,
// like a stale buffer (VolumeSampler re-bins before that can happen).
__device__ __forceinline__ bool hdr_fits(const Hdr &h, int P, int N) {  // a binning of these sizes
    return h.magic == kVolMagic && h.P == P && h.N == N;
}
// the guard of every sampling kernel: a stale buffer, or inputs that differ from the binned ones
__device__ __forceinline__ bool vol_stale(const char *buf, const Hdr &h, int P, int N) {
    return !hdr_fits(h, P, N) || *reinterpret_cast<const volatile int *>(buf + h.o_flag) != 0;
}

__global__ void k_vol_flag_reset(int P, int N, char *buf) {
    const Hdr &h = hdr_of(buf);
    if (threadIdx.x == 0 && hdr_fits(h, P, N)) *reinterpret_cast<int *>(buf + h.o_flag) = 0;
}

__global__ void k_vol_verify(int P, int N, const uint32_t *__restrict__ m, const uint32_t *__restrict__ c,
                             const uint32_t *__restrict__ sm, char *buf) {
    const Hdr h = hdr_of(buf);
    if (!hdr_fits(h, P, N)) return;  // (the kernels flag a stale buffer)
    const int64_t nm = (int64_t)P * 3, nc = (int64_t)P * 6, ns = (int64_t)N * 3;
    const uint32_t *mc = reinterpret_cast<const uint32_t *>(buf + h.o_mcopy);
    const uint32_t *cc = reinterpret_cast<const uint32_t *>(buf + h.o_ccopy);
    const uint32_t *sc = reinterpret_cast<const uint32_t *>(buf + h.o_scopy);
    bool diff = false;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nm + nc + ns; i += stride)
        diff |= i < nm ? m[i] != mc[i] : (i < nm + nc ? c[i - nm] != cc[i - nm] : sm[i - nm - nc] != sc[i - nm - nc]);
    if (__any(diff) && (threadIdx.x & (kWave - 1)) == 0) *reinterpret_cast<volatile int *>(buf + h.o_flag) = 1;
}

// count_pairs: the flag word (or 1 for a stale buffer) into out
__global__ void k_vol_flag_read(int P, int N, const char *buf, unsigned long long *out) {
    if (threadIdx.x == 0) out[0] = vol_stale(buf, hdr_of(buf), P, N) ? 1ull : 0ull;
}

__global__ void k_vol_header(Hdr h, HdrAx hx, char *buf) {
    if (threadIdx.x == 0) {
        *reinterpret_cast<Hdr *>(buf) = h;
        *reinterpret_cast<HdrAx *>(buf + sizeof(Hdr)) = hx;
    }
}

// ------------------------------------------------------------------------------ the walks
// What every sampling kernel starts with: the guard (vol_stale, above) and the binned arrays.  The
// header is read in place (const Hdr &): a local copy indexed by the axis would live in scratch.
struct Bin {  // the binned arrays of a buffer
    const int32_t *__restrict__ gids, *__restrict__ sids, *__restrict__ gstart, *__restrict__ sstart;
    const float4 *__restrict__ gpk, *__restrict__ gek;
};
__device__ __forceinline__ Bin bin_of(const char *buf, const Hdr &h) {
    return {reinterpret_cast<const int32_t *>(buf + h.o_gids),   reinterpret_cast<const int32_t *>(buf + h.o_sids),
            reinterpret_cast<const int32_t *>(buf + h.o_gstart), reinterpret_cast<const int32_t *>(buf + h.o_sstart),
            reinterpret_cast<const float4 *>(buf + h.o_gpk),     reinterpret_cast<const float4 *>(buf + h.o_gek)};
}

// Images of one axis that a box [pl, ph] of points with reach r can meet inside the grid's extent
// (HdrAx: an open axis has the direct one only).
__device__ __forceinline__ Win box_images(const HdrAx &hx, int d, float pl, float ph, float r, bool target_is_mean) {
    const Win wa = image_range(pl, r, hx.ilo[d], hx.ihi[d], target_is_mean);
    const Win wb = image_range(ph, r, hx.ilo[d], hx.ihi[d], target_is_mean);
    return {min(wa.k0, wb.k0), max(wa.k1, wb.k1)};
}
// One axis of a window: the cells [c0, c1] that the targets of the box [pl, ph] under image k and
// reach r can lie in; false when the window misses the grid.  The windows are in x = m - s, so
// means lie at p + x of a sample box and samples at p - x of a means box.
__device__ __forceinline__ bool window_cells(const Hdr &h, int d, int k, float r, float pl, float ph,
                                             bool target_is_mean, int &c0, int &c1) {
    float xa, xb;
    image_window(k, r, xa, xb);
    const float ta = target_is_mean ? pl + xa : pl - xb, tb = target_is_mean ? ph + xb : ph - xa;
    const float glo = h.lo[d], ghi = h.lo[d] + h.cs[d] * h.n[d];
    if (tb < glo || ta > ghi) return false;
    c0 = cell_axis(h, d, ta);
    c1 = cell_axis(h, d, tb);
    return true;
}
// the pair (m, s) lies inside the Gaussian's cut box r at image kk.  (&, not &&: one test of
// the three axes; short-circuited, each axis waits for its own LDS read of the staged candidate.)
__device__ __forceinline__ bool in_cut_box(const float *m, const float *s, const float *r, const int *kk) {
    bool mine = true;
    for (int d = 0; d < 3; ++d) {
        const float x = m[d] - s[d];
        mine &= fabsf(x - 2.0f * kk[d]) <= r[d] + 1e-5f;
    }
    return mine;
}

// ------------------------------------------------------------------------------ forward
// One wave per (sample cell, 64 of its samples), lane = sample.  The wave walks the image
// windows of the whole cell (reach E, the largest small-Gaussian cut): the candidates of a row
// of cells are one range of the cell-sorted Gaussians, staged 64 at a time in LDS (one
// coalesced load per lane: mean, cut widths, conic) and read back as broadcasts.  Each lane
// keeps a candidate only through the image of its own displacement and inside the candidate's
// own cut box, then evaluates the pair.  Then every big Gaussian.  Outputs summed in registers.
constexpr int kVolFwdBlocks = 8192;

template <int CB>
struct VCand {
    float4 mp;  // mean, id bits in .w
    float4 ge;  // cut half-widths
    float c[6];
    float v[CB];  // values of the launch's channel block
};

// The walk of one chunk (the wave's 64 samples s of cell cc, `active` lanes) over the small
// Gaussians: fill(v, g) sets the staged candidate's values v[CB] of Gaussian g, and
// eval(m, c, v) takes a candidate (mean, conic, staged values) that the lane keeps.
template <int CB, class Fill, class Eval>
__device__ __forceinline__ void walk_candidates(const Hdr &h, const HdrAx &hx, const Bin &bin, const float *__restrict__ conics,
                                                VCand<CB> *cand, int lane, const int *cc, bool active,
                                                const float *s, Fill fill, Eval eval) {
    if (h.nsmall <= 0) return;
    // the chunk's sample box (its cell's, widened by the rounding of the grid)
    float bl[3], bh[3];
    Win w[3];
    for (int d = 0; d < 3; ++d) {
        bl[d] = h.lo[d] + h.cs[d] * cc[d] - 1e-5f;
        bh[d] = h.lo[d] + h.cs[d] * (cc[d] + 1) + 1e-5f;
        if (cc[d] == 0) bl[d] = -INFINITY;  // (clamped cells hold everything below / above)
        if (cc[d] == h.n[d] - 1) bh[d] = INFINITY;
        float mn = INFINITY, mx = -INFINITY;
        if (active) { mn = s[d]; mx = s[d]; }
        for (int o = kWave / 2; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o));
            mx = fmaxf(mx, __shfl_xor(mx, o));
        }
        bl[d] = fmaxf(bl[d], mn);
        bh[d] = fminf(bh[d], mx);
        w[d] = box_images(hx, d, bl[d], bh[d], h.E[d], true);
    }
    for (int cls = 0; cls < 2; ++cls)  // per class: its own reach
    for (int kz = w[2].k0; kz <= w[2].k1; ++kz)
        for (int ky = w[1].k0; ky <= w[1].k1; ++ky)
            for (int kx = w[0].k0; kx <= w[0].k1; ++kx) {
                const int kk[3] = {kx, ky, kz};
                int c0[3], c1[3];
                bool any = true;
                for (int d = 0; d < 3 && any; ++d)  // the mean window
                    any = window_cells(h, d, kk[d], h.Ec[cls][d], bl[d], bh[d], true, c0[d], c1[d]);
                if (!any) continue;
                for (int cz = c0[2]; cz <= c1[2]; ++cz)
                    for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                        const int row = cls * h.ncells + (cz * h.n[1] + cy) * h.n[0];
                        const int b = bin.gstart[row + c0[0]], e = bin.gstart[row + c1[0] + 1];
                        for (int q0 = b; q0 < e; q0 += kWave) {
                            const int q = q0 + lane;
                            __syncthreads();
                            if (q < e) {
                                VCand<CB> v;
                                v.mp = bin.gpk[q];
                                v.ge = bin.gek[q];
                                const int g = __float_as_int(v.mp.w);
                                for (int k = 0; k < 6; ++k) v.c[k] = conics[(int64_t)g * 6 + k];
                                fill(v.v, g);
                                cand[lane] = v;
                            }
                            __syncthreads();
                            const int cnt = min(kWave, e - q0);
                            if (active)
                                for (int u = 0; u < cnt; ++u) {
                                    const float4 mp = cand[u].mp, ge = cand[u].ge;
                                    const float m[3] = {mp.x, mp.y, mp.z};
                                    const float r[3] = {ge.x, ge.y, ge.z};
                                    if (in_cut_box(m, s, r, kk)) eval(m, cand[u].c, cand[u].v);
                                }
                        }
                    }
            }
}

template <int FN, int CB>  // (with the _mc kernels, below)
__device__ __forceinline__ void fwd_acc_c(int nch, const float *vr, float G, const float *a, const float *c,
                                          float (*acc)[CB], const float *cf = nullptr);

// The C > 1 forward (C = 1: k_vol_forward_m), CB channels per launch.  COUNT (diagnostic,
// dgs_volume_count_pairs): instead of the outputs, counts[0] += the pairs evaluated (candidates
// inside their cut box) and counts[1] += the live ones (G > 0).  CF: VCoef for the operator, else
// empty (as in every kernel below that has it).
template <int FN, int CB, bool COUNT = false, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_forward(const char *__restrict__ buf, int P, int N, int C, int cbase,
                                                       const float *__restrict__ means,
                                                       const float *__restrict__ values,
                                                       const float *__restrict__ conics,
                                                       const float *__restrict__ samples, float *__restrict__ out,
                                                       unsigned long long *__restrict__ counts = nullptr,
                                                       CF... coef) {
    constexpr int KU = VTr<FN>::KU, K = VTr<FN>::K;
    const float *cf = coef_of(coef...);
    __shared__ VCand<CB> cand[kWave];
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    const int nch = min(CB, C - cbase);
    if (vol_stale(buf, h, P, N)) {
        if (COUNT) return;
        for (int64_t j = (int64_t)blockIdx.x * kWave + lane; j < N; j += (int64_t)gridDim.x * kWave)
            for (int f = 0; f < K; ++f)
                for (int ch = 0; ch < nch; ++ch) out[(j * K + f) * C + cbase + ch] = NAN;
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < h.ncells; cell += gridDim.x) {
        const int sb = bin.sstart[cell], se = bin.sstart[cell + 1];
        const int cc[3] = {cell % h.n[0], (cell / h.n[0]) % h.n[1], cell / (h.n[0] * h.n[1])};
        for (int j0 = sb; j0 < se; j0 += kWave) {
            const int j = j0 + lane;
            const bool active = j < se;
            const int sid = active ? bin.sids[j] : 0;
            float s[3];
            for (int d = 0; d < 3; ++d) s[d] = active ? samples[(int64_t)sid * 3 + d] : 0.0f;
            float acc[KU][CB];
            for (int u = 0; u < KU; ++u)
                for (int ch = 0; ch < CB; ++ch) acc[u][ch] = 0.0f;
            unsigned long long n_cand = 0, n_live = 0;
            auto values_of = [&](float *vr, int g) {
                for (int ch = 0; ch < CB; ++ch) vr[ch] = ch < nch ? values[(int64_t)g * C + cbase + ch] : 0.0f;
            };
            auto eval = [&](const auto &ax, const float *m, const float *c, const float *vr) {
                float X[3], a[3], G, t[KU];
                if constexpr (COUNT) {
                    ++n_cand;
                    if (pair_eval(ax, m, s, c, X, G, a)) ++n_live;
                    return;
                }
                if (!pair_eval(ax, m, s, c, X, G, a)) return;
                if constexpr (FN == kFnTrace) {  // no legacy bits to keep: the written-out sum (fwd_acc_c)
                    fwd_acc_c<FN, CB>(nch, vr, G, a, c, acc);
                    return;
                }
                if constexpr (FN == kFnOp) {  // (likewise)
                    fwd_acc_c<FN, CB>(nch, vr, G, a, c, acc, cf);
                    return;
                }
                terms<FN>(a, c, t);
                for (int ch = 0; ch < nch; ++ch) {
                    const float v = vr[ch];
                    for (int u = 0; u < KU; ++u) acc[u][ch] += v * G * t[u];
                }
            };
            walk_candidates<CB>(h, hax_of(buf), bin, conics, cand, lane, cc, active, s, values_of,
                                [&](const float *m, const float *c, const float *vr) { eval(Torus{}, m, c, vr); });
            if (active) {
                const Axes ax = axes_of(buf);  // (the big Gaussians meet every sample: pair_eval needs the axes)
                for (int q = bin.gstart[2 * h.ncells]; q < bin.gstart[2 * h.ncells + 1]; ++q) {  // big ones
                    const int g = bin.gids[q];
                    float m[3], c[6], vr[CB];
                    for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
                    for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                    values_of(vr, g);
                    eval(ax, m, c, vr);
                }
                if constexpr (COUNT) {
                    atomicAdd(&counts[0], n_cand);
                    atomicAdd(&counts[1], n_live);
                } else {
                    for (int f = 0; f < K; ++f) {
                        const int u = umap<FN>(f);
                        for (int ch = 0; ch < nch; ++ch) out[((int64_t)sid * K + f) * C + cbase + ch] = acc[u][ch];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------ backward
// hs[sid][u][ch]: dL summed over the full components that share unique component u
template <int FN>
__global__ __launch_bounds__(kBlock) void k_vol_hsum(int N, int C, const float *__restrict__ dL, float *__restrict__ hs) {
    constexpr int KU = VTr<FN>::KU, K = VTr<FN>::K;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)N * C) return;
    const int64_t sid = t / C;
    const int ch = (int)(t - sid * C);
    float h[KU];
    for (int u = 0; u < KU; ++u) h[u] = 0.0f;
#pragma unroll
    for (int f = 0; f < K; ++f) h[umap<FN>(f)] += dL[(sid * K + f) * C + ch];
    for (int u = 0; u < KU; ++u) hs[(sid * KU + u) * C + ch] = h[u];
}

// One pair's contribution to a Gaussian's gradient sums.  hrow: the sample's h row [KU][C]
// (global).  CB == 1 means C == 1 (the big Gaussians): phi, g and e are
// linear in h v0, so the pair uses h alone and the caller scales the mean / conic sums by v0 once
// (bwd_store's scale).
template <int FN, int CB, class AX>
__device__ __forceinline__ void bwd_pair(const AX &ax, const float *m, const float *c, const float *__restrict__ values, int g,
                                         int C, int cbase, int nch, const float *s, const float *hrow,
                                         float *dm, float *dc, float *dv, const float *cf = nullptr) {
    constexpr int KU = VTr<FN>::KU;
    float X[3], a[3], G, t[KU];
    if (!pair_eval(ax, m, s, c, X, G, a)) return;
    terms<FN>(a, c, t, cf);
    float hv[KU];
    if constexpr (CB == 1) {
        float p = 0.0f;
        for (int u = 0; u < KU; ++u) p += hrow[u] * t[u];
        dv[0] += G * p;
        float gg[3], e[6];
        phi_grads<FN>(hrow, a, c, gg, e, cf);
        pair_grads(G, p, X, a, c, gg, e, dm, dc);
        return;
    } else {
        for (int u = 0; u < KU; ++u) hv[u] = 0.0f;
        for (int ch = 0; ch < C; ++ch) {
            const float v = values[(int64_t)g * C + ch];
            for (int u = 0; u < KU; ++u) hv[u] += v * hrow[u * C + ch];
        }
        for (int ch = 0; ch < nch; ++ch) {
            float p = 0.0f;
            for (int u = 0; u < KU; ++u) p += hrow[u * C + cbase + ch] * t[u];
            dv[ch] += G * p;
        }
    }
    float phi = 0.0f;
    for (int u = 0; u < KU; ++u) phi += hv[u] * t[u];
    float gg[3], e[6];
    phi_grads<FN>(hv, a, c, gg, e, cf);
    pair_grads(G, phi, X, a, c, gg, e, dm, dc);
}

// ---- C = 1: the moment (tensor) form of the backward (the D = 2 form of 4.3b in
// three dimensions).  With the sample's h scaled to the full symmetric tensor H (h_u divided by
// the multiplicity of its index set, at staging), phi = sum_u h_u t_u and its partials are
//   laplacian: phi = a.(H a) - H:c,          g = 2 H a,          e = -H (packed, off-diagonals x2)
//   trace    : phi = H (a.a - tr c),         g = 2 H a,          e = -H on the diagonal (H a scalar)
//   operator : phi = H t (op_t),             g = H (b + 2 W a),  e = -H m_u w_u          (H a scalar)
//   third    : E_pq = H_pqk a_k, M = E a,     w_k = c_ij H_ijk,
//              phi = 3 w.a - M.a,            g = 3 (w - M),      e = 3 E (off-diagonals x2)
// and the pair only adds moments: G phi, G g, G phi X, G phi X X^T, G (g X^T + X g^T), G e.  The
// Gaussian's gradients follow once per lane (vol_mom_finish): dm = A (sum G g - sum G phi X),
// dc = -1/2 sum G phi XX (off-diagonal -1) + sum G gX + sum G e, dv = sum G phi.  About 130
// flops per pair for the third against ~300 for the per-pair terms (bwd_pair).
struct VMom {
    float sphi, sg[3], spx[3], spxx[6], sgx[6], se[6];
};

template <int FN>
__host__ __device__ constexpr float vol_inv_mult(int u) {
    if (FN == 2) return (u == 0 || u == 3 || u == 5) ? 1.0f : 0.5f;
    if (FN == 3) return (u == 0 || u == 6 || u == 9) ? 1.0f : (u == 4 ? 1.0f / 6.0f : 1.0f / 3.0f);
    return 1.0f;
}

// phi, g = d phi / d a and e = d phi / d c (packed) of one function from the sample's tensor H.
// Entries a function does not have (g of the gaussian, e below the laplacian) are left as given.
template <int FN>
__device__ __forceinline__ void phi_ge_t(const float *H, const float *a, const float *c2, float &phi, float *g,
                                         float *e, const float *cf = nullptr) {
    if constexpr (FN == 0) {
        phi = H[0];
    } else if constexpr (FN == 1) {
        phi = H[0] * a[0] + H[1] * a[1] + H[2] * a[2];
        g[0] = H[0]; g[1] = H[1]; g[2] = H[2];
    } else if constexpr (FN == 2) {
        const float ha0 = H[0] * a[0] + H[1] * a[1] + H[2] * a[2];
        const float ha1 = H[1] * a[0] + H[3] * a[1] + H[4] * a[2];
        const float ha2 = H[2] * a[0] + H[4] * a[1] + H[5] * a[2];
        float hc = 0.0f;
#pragma unroll
        for (int q = 0; q < 6; ++q) hc += H[q] * c2[q];
        phi = a[0] * ha0 + a[1] * ha1 + a[2] * ha2 - hc;
        g[0] = 2.0f * ha0; g[1] = 2.0f * ha1; g[2] = 2.0f * ha2;
        e[0] = -H[0]; e[1] = -2.0f * H[1]; e[2] = -2.0f * H[2]; e[3] = -H[3]; e[4] = -2.0f * H[4]; e[5] = -H[5];
    } else if constexpr (FN == kFnTrace) {  // the laplacian's with H = H[0] I
        phi = H[0] * ((a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) - (c2[0] + c2[3] + c2[5]));
        const float h2 = 2.0f * H[0];
        g[0] = h2 * a[0]; g[1] = h2 * a[1]; g[2] = h2 * a[2];
        e[0] = -H[0]; e[3] = -H[0]; e[5] = -H[0];
    } else if constexpr (FN == kFnOp) {
        phi = H[0] * op_t(a, c2, cf, 0.5f);
        op_ge(H[0], a, cf, g, e);
    } else {
        // H000 H001 H002 H011 H012 H022 H111 H112 H122 H222 = H[0..9]
        const float E00 = H[0] * a[0] + H[1] * a[1] + H[2] * a[2];
        const float E01 = H[1] * a[0] + H[3] * a[1] + H[4] * a[2];
        const float E02 = H[2] * a[0] + H[4] * a[1] + H[5] * a[2];
        const float E11 = H[3] * a[0] + H[6] * a[1] + H[7] * a[2];
        const float E12 = H[4] * a[0] + H[7] * a[1] + H[8] * a[2];
        const float E22 = H[5] * a[0] + H[8] * a[1] + H[9] * a[2];
        const float M0 = E00 * a[0] + E01 * a[1] + E02 * a[2];
        const float M1 = E01 * a[0] + E11 * a[1] + E12 * a[2];
        const float M2 = E02 * a[0] + E12 * a[1] + E22 * a[2];
        // c2 = [c00 2c01 2c02 c11 2c12 c22]
        const float w0 = c2[0] * H[0] + c2[3] * H[3] + c2[5] * H[5] + c2[1] * H[1] + c2[2] * H[2] + c2[4] * H[4];
        const float w1 = c2[0] * H[1] + c2[3] * H[6] + c2[5] * H[8] + c2[1] * H[3] + c2[2] * H[4] + c2[4] * H[7];
        const float w2 = c2[0] * H[2] + c2[3] * H[7] + c2[5] * H[9] + c2[1] * H[4] + c2[2] * H[5] + c2[4] * H[8];
        phi = 3.0f * (w0 * a[0] + w1 * a[1] + w2 * a[2]) - (M0 * a[0] + M1 * a[1] + M2 * a[2]);
        g[0] = 3.0f * (w0 - M0); g[1] = 3.0f * (w1 - M1); g[2] = 3.0f * (w2 - M2);
        e[0] = 3.0f * E00; e[1] = 6.0f * E01; e[2] = 6.0f * E02; e[3] = 3.0f * E11; e[4] = 6.0f * E12; e[5] = 3.0f * E22;
    }
}

// Adds one pair's moments for phi, g, e of function order up to TOP (g from 1, e from 2).
template <int TOP>
__device__ __forceinline__ void vol_mom_add(float G, float phi, const float *g, const float *e, const float *X,
                                            VMom &M) {
    const float Gp = G * phi;
    M.sphi += Gp;
    const float XX[6] = {X[0] * X[0], X[0] * X[1], X[0] * X[2], X[1] * X[1], X[1] * X[2], X[2] * X[2]};
#pragma unroll
    for (int d = 0; d < 3; ++d) M.spx[d] += Gp * X[d];
#pragma unroll
    for (int q = 0; q < 6; ++q) M.spxx[q] += Gp * XX[q];
    if constexpr (TOP >= 1) {
        const float Gg[3] = {G * g[0], G * g[1], G * g[2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) M.sg[d] += Gg[d];
        M.sgx[0] += Gg[0] * X[0];
        M.sgx[1] += Gg[0] * X[1] + Gg[1] * X[0];
        M.sgx[2] += Gg[0] * X[2] + Gg[2] * X[0];
        M.sgx[3] += Gg[1] * X[1];
        M.sgx[4] += Gg[1] * X[2] + Gg[2] * X[1];
        M.sgx[5] += Gg[2] * X[2];
    }
    if constexpr (TOP >= 2) {
#pragma unroll
        for (int q = 0; q < 6; ++q) M.se[q] += G * e[q];
    }
}

template <int FN, class AX>
__device__ __forceinline__ void bwd_pair_t(const AX &ax, const float *m, const float *c, const float *c2, const float *s,
                                           const float *H, VMom &M) {
    float X[3], a[3], G;
    if (!pair_eval(ax, m, s, c, X, G, a)) return;
    float phi, g[3] = {0.0f, 0.0f, 0.0f}, e[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    phi_ge_t<FN>(H, a, c2, phi, g, e);
    vol_mom_add<mask_top(1 << FN)>(G, phi, g, e, X, M);
}

__device__ __forceinline__ void vol_mom_finish(const float *c, const VMom &M, float *dm, float *dc, float *dv) {
    const float d[3] = {M.sg[0] - M.spx[0], M.sg[1] - M.spx[1], M.sg[2] - M.spx[2]};
    dm[0] = c[0] * d[0] + c[1] * d[1] + c[2] * d[2];
    dm[1] = c[1] * d[0] + c[3] * d[1] + c[4] * d[2];
    dm[2] = c[2] * d[0] + c[4] * d[1] + c[5] * d[2];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const bool diag = q == 0 || q == 3 || q == 5;
        dc[q] = (diag ? -0.5f : -1.0f) * M.spxx[q] + M.sgx[q] + M.se[q];
    }
    dv[0] = M.sphi;
}

template <int CB>
__device__ __forceinline__ void bwd_store(int g, int C, int cbase, int nch, const float *dm, const float *dc,
                                          const float *dv, float *__restrict__ dmeans, float *__restrict__ dvalues,
                                          float *__restrict__ dconics, float scale = 1.0f) {
    if (cbase == 0) {
        for (int d = 0; d < 3; ++d) dmeans[(int64_t)g * 3 + d] = scale * dm[d];
        for (int q = 0; q < 6; ++q) dconics[(int64_t)g * 6 + q] = scale * dc[q];
    }
    for (int ch = 0; ch < nch; ++ch) dvalues[(int64_t)g * C + cbase + ch] = dv[ch];
}

// One wave per (Gaussian cell, 64 of its small Gaussians), lane = Gaussian.  The wave walks
// the image windows of its Gaussians' union (means box, largest cut among them): the samples of
// a row of cells are one range of the cell-sorted samples, staged 64 at a time in LDS (one
// coalesced load per lane) and read back as broadcasts.  Each lane keeps a sample only through
// the image of its own displacement and inside its own cut box; gradients summed in registers
// and written once (no atomics).
constexpr int kVolBwdBlocks = 8192;

template <int FN, int CB, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_backward(const char *__restrict__ buf, int P, int N, int C, int cbase,
                                                        const float *__restrict__ means,
                                                        const float *__restrict__ values,
                                                        const float *__restrict__ conics,
                                                        const float *__restrict__ samples,
                                                        const float *__restrict__ hs, float *__restrict__ dmeans,
                                                        float *__restrict__ dvalues, float *__restrict__ dconics,
                                                        CF... coef) {
    constexpr int KU = VTr<FN>::KU;
    const float *cf = coef_of(coef...);
    __shared__ float4 scand[kWave];
    __shared__ float shrow[kWave][CB == 1 ? KU : 1];  // C == 1: the candidates' h rows
    const Hdr h = hdr_of(buf);
    const int lane = threadIdx.x;
    const int nch = min(CB, C - cbase);
    if (vol_stale(buf, h, P, N)) {  // stale buffer / inputs: loud
        const float nan[9] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};
        for (int64_t i = (int64_t)blockIdx.x * kWave + lane; i < P; i += (int64_t)gridDim.x * kWave)
            bwd_store<CB>((int)i, C, cbase, nch, nan, nan, nan, dmeans, dvalues, dconics);
        return;
    }
    const int32_t *__restrict__ gids = reinterpret_cast<const int32_t *>(buf + h.o_gids);
    const int32_t *__restrict__ sids = reinterpret_cast<const int32_t *>(buf + h.o_sids);
    const int32_t *__restrict__ gstart = reinterpret_cast<const int32_t *>(buf + h.o_gstart);
    const int32_t *__restrict__ sstart = reinterpret_cast<const int32_t *>(buf + h.o_sstart);
    const float4 *__restrict__ gpk = reinterpret_cast<const float4 *>(buf + h.o_gpk);
    const float4 *__restrict__ gek = reinterpret_cast<const float4 *>(buf + h.o_gek);
    for (int cell = blockIdx.x; cell < 2 * h.ncells; cell += gridDim.x) {  // (class-major cells)
        const int gb = gstart[cell], ge = gstart[cell + 1];
        for (int i0 = gb; i0 < ge; i0 += kWave) {
            const int i = i0 + lane;
            const bool active = i < ge;
            float m[3] = {0.0f, 0.0f, 0.0f}, r[3] = {0.0f, 0.0f, 0.0f}, c[6];
            int g = 0;
            float v0 = 0.0f;
            if (active) {
                const float4 mp = gpk[i], ex = gek[i];
                g = __float_as_int(mp.w);
                if constexpr (CB == 1) v0 = values[g];
                m[0] = mp.x; m[1] = mp.y; m[2] = mp.z;
                r[0] = ex.x; r[1] = ex.y; r[2] = ex.z;
                for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
            } else {
                for (int k = 0; k < 6; ++k) c[k] = 0.0f;
            }
            float dm[3] = {0.0f, 0.0f, 0.0f}, dc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, dv[CB];
            for (int ch = 0; ch < CB; ++ch) dv[ch] = 0.0f;
            VMom mom{};  // CB == 1: the moment form
            const float c2[6] = {c[0], 2.0f * c[1], 2.0f * c[2], c[3], 2.0f * c[4], c[5]};
            float ml[3], mh[3], R[3];
            Win w[3];
            for (int d = 0; d < 3; ++d) {
                float mn = active ? m[d] : INFINITY, mx = active ? m[d] : -INFINITY, rr = r[d];
                for (int o = kWave / 2; o > 0; o >>= 1) {
                    mn = fminf(mn, __shfl_xor(mn, o));
                    mx = fmaxf(mx, __shfl_xor(mx, o));
                    rr = fmaxf(rr, __shfl_xor(rr, o));
                }
                ml[d] = mn; mh[d] = mx; R[d] = rr;
                const HdrAx &hx = hax_of(buf);  // (an open axis: the direct image only)
                const Win wa = image_range(mn, rr, hx.ilo[d], hx.ihi[d], false);
                const Win wb = image_range(mx, rr, hx.ilo[d], hx.ihi[d], false);
                w[d].k0 = min(wa.k0, wb.k0);
                w[d].k1 = max(wa.k1, wb.k1);
            }
            for (int kz = w[2].k0; kz <= w[2].k1; ++kz)
                for (int ky = w[1].k0; ky <= w[1].k1; ++ky)
                    for (int kx = w[0].k0; kx <= w[0].k1; ++kx) {
                        const int kk[3] = {kx, ky, kz};
                        int c0[3], c1[3];
                        bool any = true;
                        for (int d = 0; d < 3; ++d) {
                            float xa, xb;
                            image_window(kk[d], R[d], xa, xb);
                            const float ta = ml[d] - xb, tb = mh[d] - xa;  // sample window
                            const float glo = h.lo[d], ghi = h.lo[d] + h.cs[d] * h.n[d];
                            if (tb < glo || ta > ghi) { any = false; break; }
                            c0[d] = cell_axis(h, d, ta);
                            c1[d] = cell_axis(h, d, tb);
                        }
                        if (!any) continue;
                        for (int cz = c0[2]; cz <= c1[2]; ++cz)
                            for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                                const int row = (cz * h.n[1] + cy) * h.n[0];
                                const int b = sstart[row + c0[0]], e = sstart[row + c1[0] + 1];
                                for (int q0 = b; q0 < e; q0 += kWave) {
                                    const int q = q0 + lane;
                                    __syncthreads();
                                    if (q < e) {
                                        const int sid = sids[q];
                                        scand[lane] = make_float4(samples[(int64_t)sid * 3], samples[(int64_t)sid * 3 + 1],
                                                                  samples[(int64_t)sid * 3 + 2], __int_as_float(sid));
                                        if constexpr (CB == 1)  // the tensor H (bwd_pair_t)
                                            for (int u = 0; u < KU; ++u)
                                                shrow[lane][u] = hs[(int64_t)sid * KU + u] * vol_inv_mult<FN>(u);
                                    }
                                    __syncthreads();
                                    const int cnt = min(kWave, e - q0);
                                    if (active)
                                        for (int u = 0; u < cnt; ++u) {
                                            const float4 sp = scand[u];
                                            const float sv[3] = {sp.x, sp.y, sp.z};
                                            bool mine = true;
                                            for (int d = 0; d < 3; ++d) {  // inside its cut box at image kk
                                                const float x = m[d] - sv[d];
                                                mine = mine && fabsf(x - 2.0f * kk[d]) <= r[d] + 1e-5f;
                                            }
                                            if (mine) {
                                                if constexpr (CB == 1)
                                                    bwd_pair_t<FN>(Torus{}, m, c, c2, sv, &shrow[u][0], mom);
                                                else
                                                    bwd_pair<FN, CB>(Torus{}, m, c, values, g, C, cbase, nch, sv,
                                                                     hs + (int64_t)__float_as_int(sp.w) * KU * C, dm,
                                                                     dc, dv, cf);
                                            }
                                        }
                                }
                            }
                    }
            if constexpr (CB == 1) vol_mom_finish(c, mom, dm, dc, dv);
            if (active) bwd_store<CB>(g, C, cbase, nch, dm, dc, dv, dmeans, dvalues, dconics, CB == 1 ? v0 : 1.0f);
        }
    }
}

// Big Gaussians: one block each, threads striding over every sample, block sums.
template <int FN, int CB, class... CF>
__global__ __launch_bounds__(kBlock) void k_vol_backward_big(const char *__restrict__ buf, int P, int N, int C,
                                                             int cbase, const float *__restrict__ means,
                                                             const float *__restrict__ values,
                                                             const float *__restrict__ conics,
                                                             const float *__restrict__ samples,
                                                             const float *__restrict__ hs,
                                                             float *__restrict__ dmeans,
                                                             float *__restrict__ dvalues,
                                                             float *__restrict__ dconics, CF... coef) {
    constexpr int NV = 9 + CB;
    const float *cf = coef_of(coef...);
    __shared__ float part[kWavesPerBlock][NV];
    const Hdr h = hdr_of(buf);
    if (vol_stale(buf, h, P, N)) return;  // (k_vol_backward writes the NaN)
    const Axes ax = axes_of(buf);
    const int32_t *__restrict__ gids = reinterpret_cast<const int32_t *>(buf + h.o_gids);
    const int nch = min(CB, C - cbase);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    for (int b = blockIdx.x; b < h.nbig; b += gridDim.x) {
        const int g = gids[h.nsmall + b];
        float m[3], c[6];
        for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
        for (int q = 0; q < 6; ++q) c[q] = conics[(int64_t)g * 6 + q];
        float v[NV];
        for (int k = 0; k < NV; ++k) v[k] = 0.0f;
        for (int sid = threadIdx.x; sid < N; sid += kBlock) {
            const float sp[3] = {samples[(int64_t)sid * 3], samples[(int64_t)sid * 3 + 1], samples[(int64_t)sid * 3 + 2]};
            bwd_pair<FN, CB>(ax, m, c, values, g, C, cbase, nch, sp,
                             hs + (int64_t)sid * VTr<FN>::KU * C, v, v + 3, v + 9, cf);
        }
        for (int k = 0; k < NV; ++k)
            for (int o = kWave / 2; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
        if (lane == 0)
            for (int k = 0; k < NV; ++k) part[w][k] = v[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            float t[NV];
            for (int k = 0; k < NV; ++k) {
                t[k] = 0.0f;
                for (int q = 0; q < kWavesPerBlock; ++q) t[k] += part[q][k];
            }
            bwd_store<CB>(g, C, cbase, nch, t, t + 3, t + 9, dmeans, dvalues, dconics, CB == 1 ? values[g] : 1.0f);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------ C = 1: function masks
// One or several of the four functions of one field at the same samples (C = 1; DESIGN.md 4.8,
// "fused functions"): one walk of the candidates, one pair_eval per kept pair, for every function
// of MASK (bit f = function f).  The single-function forward at C = 1 is the single-bit mask, so
// a fused output equals the single call's by construction; the backward of one function is
// k_vol_backward<FN, 1>, of several k_vol_backward_m.
struct VOuts {
    float *p[4];  // per function code (fn_slot: the trace in the laplacian's); entries outside the mask unused
};

// acc[u] += v G t_u for function FN: the definition of the C = 1 forward sum, with every rounding
// written out so that it does not depend on what else the kernel computes (the other functions
// of a mask share v, G and a).  Among the staged candidates the sum is fma(v, G, acc) for the
// gaussian and fma(round(v G), t_u, acc) for the others; among the big Gaussians (BIG) the
// product round(round(v G) t_u) is rounded on its own and then added.
template <int FN, bool BIG>
__device__ __forceinline__ void fwd_acc(float v, float G, const float *a, const float *c, float *acc,
                                        const float *cf = nullptr) {
    constexpr int KU = VTr<FN>::KU;
    float t[KU];
    terms<FN>(a, c, t, cf);
    if constexpr (BIG) {
        const float vG = rmul(v, G);
        for (int u = 0; u < KU; ++u) acc[u] = radd(acc[u], rmul(vG, t[u]));
    } else if constexpr (FN == 0) {
        acc[0] = __builtin_fmaf(v, G, acc[0]);
    } else {
        const float vG = rmul(v, G);
        for (int u = 0; u < KU; ++u) acc[u] = __builtin_fmaf(vG, t[u], acc[u]);
    }
}
template <int FN>
__device__ __forceinline__ void fwd_store(float *__restrict__ out, int64_t sid, const float *acc) {
    constexpr int K = VTr<FN>::K;
    for (int f = 0; f < K; ++f) out[sid * K + f] = acc[umap<FN>(f)];
}
template <int FN>
__device__ __forceinline__ void fwd_nan(float *__restrict__ out, int64_t sid) {
    constexpr int K = VTr<FN>::K;
    for (int f = 0; f < K; ++f) out[sid * K + f] = NAN;
}

template <int MASK, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_forward_m(const char *__restrict__ buf, int P, int N,
                                                         const float *__restrict__ means,
                                                         const float *__restrict__ values,
                                                         const float *__restrict__ conics,
                                                         const float *__restrict__ samples, VOuts outs,
                                                         CF... coef) {
    constexpr int SKU = mask_ku(MASK);
    constexpr int O0 = mask_off(MASK, 0), O1 = mask_off(MASK, 1), O2 = mask_off(MASK, 2), O3 = mask_off(MASK, 3);
    constexpr int O4 = mask_off(MASK, kFnTrace), S4 = fn_slot(kFnTrace);
    constexpr int O5 = mask_off(MASK, kFnOp), S5 = fn_slot(kFnOp);
    const float *cf = coef_of(coef...);
    __shared__ VCand<1> cand[kWave];
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    if (vol_stale(buf, h, P, N)) {
        for (int64_t j = (int64_t)blockIdx.x * kWave + lane; j < N; j += (int64_t)gridDim.x * kWave) {
            if constexpr ((MASK & 1) != 0) fwd_nan<0>(outs.p[0], j);
            if constexpr ((MASK & 2) != 0) fwd_nan<1>(outs.p[1], j);
            if constexpr ((MASK & 4) != 0) fwd_nan<2>(outs.p[2], j);
            if constexpr ((MASK & 8) != 0) fwd_nan<3>(outs.p[3], j);
            if constexpr ((MASK & 16) != 0) fwd_nan<kFnTrace>(outs.p[S4], j);
            if constexpr ((MASK & 32) != 0) fwd_nan<kFnOp>(outs.p[S5], j);
        }
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < h.ncells; cell += gridDim.x) {
        const int sb = bin.sstart[cell], se = bin.sstart[cell + 1];
        const int cc[3] = {cell % h.n[0], (cell / h.n[0]) % h.n[1], cell / (h.n[0] * h.n[1])};
        for (int j0 = sb; j0 < se; j0 += kWave) {
            const int j = j0 + lane;
            const bool active = j < se;
            const int sid = active ? bin.sids[j] : 0;
            float s[3];
            for (int d = 0; d < 3; ++d) s[d] = active ? samples[(int64_t)sid * 3 + d] : 0.0f;
            float acc[SKU];
            for (int u = 0; u < SKU; ++u) acc[u] = 0.0f;
            auto eval = [&](const auto &ax, const float *m, const float *c, float v, auto big) {
                constexpr bool BIG = decltype(big)::value;
                float X[3], a[3], G;
                if (!pair_eval(ax, m, s, c, X, G, a)) return;
                if constexpr ((MASK & 1) != 0) fwd_acc<0, BIG>(v, G, a, c, acc + O0);
                if constexpr ((MASK & 2) != 0) fwd_acc<1, BIG>(v, G, a, c, acc + O1);
                if constexpr ((MASK & 4) != 0) fwd_acc<2, BIG>(v, G, a, c, acc + O2);
                if constexpr ((MASK & 8) != 0) fwd_acc<3, BIG>(v, G, a, c, acc + O3);
                if constexpr ((MASK & 16) != 0) fwd_acc<kFnTrace, BIG>(v, G, a, c, acc + O4);
                if constexpr ((MASK & 32) != 0) fwd_acc<kFnOp, BIG>(v, G, a, c, acc + O5, cf);
            };
            walk_candidates<1>(
                h, hax_of(buf), bin, conics, cand, lane, cc, active, s, [&](float *vr, int g) { vr[0] = values[g]; },
                [&](const float *m, const float *c, const float *vr) { eval(Torus{}, m, c, vr[0], std::false_type{}); });
            if (active) {
                const Axes ax = axes_of(buf);  // (the big Gaussians meet every sample: pair_eval needs the axes)
                for (int q = bin.gstart[2 * h.ncells]; q < bin.gstart[2 * h.ncells + 1]; ++q) {  // big ones
                    const int g = bin.gids[q];
                    float m[3], c[6];
                    for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
                    for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                    eval(ax, m, c, values[g], std::true_type{});
                }
                if constexpr ((MASK & 1) != 0) fwd_store<0>(outs.p[0], sid, acc + O0);
                if constexpr ((MASK & 2) != 0) fwd_store<1>(outs.p[1], sid, acc + O1);
                if constexpr ((MASK & 4) != 0) fwd_store<2>(outs.p[2], sid, acc + O2);
                if constexpr ((MASK & 8) != 0) fwd_store<3>(outs.p[3], sid, acc + O3);
                if constexpr ((MASK & 16) != 0) fwd_store<kFnTrace>(outs.p[S4], sid, acc + O4);
                if constexpr ((MASK & 32) != 0) fwd_store<kFnOp>(outs.p[S5], sid, acc + O5);
            }
        }
    }
}

// k_vol_hsum at C = 1 into function FN's slice of the concatenated rows hs[N][stride]
template <int FN>
__global__ __launch_bounds__(kBlock) void k_vol_hsum_cat(int N, const float *__restrict__ dL, float *__restrict__ hs,
                                                         int stride, int off) {
    constexpr int KU = VTr<FN>::KU, K = VTr<FN>::K;
    const int64_t sid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (sid >= N) return;
    float h[KU];
    for (int u = 0; u < KU; ++u) h[u] = 0.0f;
#pragma unroll
    for (int f = 0; f < K; ++f) h[umap<FN>(f)] += dL[sid * K + f];
    for (int u = 0; u < KU; ++u) hs[sid * stride + off + u] = h[u];
}

// function FN's slice of a staged row: the tensor H of phi_ge_t
template <int FN>
__device__ __forceinline__ void stage_h(float *row, const float *__restrict__ hrow) {
    for (int u = 0; u < VTr<FN>::KU; ++u) row[u] = hrow[u] * vol_inv_mult<FN>(u);
}
// phi, g and e of function FN added to the pair's sums
template <int FN>
__device__ __forceinline__ void phi_ge_add(const float *H, const float *a, const float *c2, float &phi, float *g,
                                           float *e, const float *cf = nullptr) {
    float p, gf[3] = {0.0f, 0.0f, 0.0f}, ef[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    phi_ge_t<FN>(H, a, c2, p, gf, ef, cf);
    phi += p;
    if constexpr (FN >= 1)
        for (int d = 0; d < 3; ++d) g[d] += gf[d];
    if constexpr (FN >= 2)
        for (int q = 0; q < 6; ++q) e[q] += ef[q];
}

template <int MASK, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_backward_m(const char *__restrict__ buf, int P, int N,
                                                          const float *__restrict__ means,
                                                          const float *__restrict__ values,
                                                          const float *__restrict__ conics,
                                                          const float *__restrict__ samples,
                                                          const float *__restrict__ hs, float *__restrict__ dmeans,
                                                          float *__restrict__ dvalues, float *__restrict__ dconics,
                                                          CF... coef) {
    constexpr int SKU = mask_ku(MASK), TOP = mask_top(MASK);
    constexpr int O0 = mask_off(MASK, 0), O1 = mask_off(MASK, 1), O2 = mask_off(MASK, 2), O3 = mask_off(MASK, 3);
    constexpr int O4 = mask_off(MASK, kFnTrace), S4 = fn_slot(kFnTrace);
    constexpr int O5 = mask_off(MASK, kFnOp);
    const float *cf = coef_of(coef...);
    __shared__ float4 scand[kWave];
    __shared__ float shrow[kWave][SKU];  // the candidates' H rows, function after function
    const Hdr &h = hdr_of(buf);  // (in place, as k_vol_forward_m)
    const int lane = threadIdx.x;
    if (vol_stale(buf, h, P, N)) {  // stale buffer / inputs: loud
        const float nan[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
        for (int64_t i = (int64_t)blockIdx.x * kWave + lane; i < P; i += (int64_t)gridDim.x * kWave)
            bwd_store<1>((int)i, 1, 0, 1, nan, nan, nan, dmeans, dvalues, dconics);
        return;
    }
    const int32_t *__restrict__ sids = reinterpret_cast<const int32_t *>(buf + h.o_sids);
    const int32_t *__restrict__ gstart = reinterpret_cast<const int32_t *>(buf + h.o_gstart);
    const int32_t *__restrict__ sstart = reinterpret_cast<const int32_t *>(buf + h.o_sstart);
    const float4 *__restrict__ gpk = reinterpret_cast<const float4 *>(buf + h.o_gpk);
    const float4 *__restrict__ gek = reinterpret_cast<const float4 *>(buf + h.o_gek);
    for (int cell = blockIdx.x; cell < 2 * h.ncells; cell += gridDim.x) {  // (class-major cells)
        const int gb = gstart[cell], ge = gstart[cell + 1];
        for (int i0 = gb; i0 < ge; i0 += kWave) {
            const int i = i0 + lane;
            const bool active = i < ge;
            float m[3] = {0.0f, 0.0f, 0.0f}, r[3] = {0.0f, 0.0f, 0.0f}, c[6];
            int g = 0;
            float v0 = 0.0f;
            if (active) {
                const float4 mp = gpk[i], ex = gek[i];
                g = __float_as_int(mp.w);
                v0 = values[g];
                m[0] = mp.x; m[1] = mp.y; m[2] = mp.z;
                r[0] = ex.x; r[1] = ex.y; r[2] = ex.z;
                for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
            } else {
                for (int k = 0; k < 6; ++k) c[k] = 0.0f;
            }
            VMom mom{};
            const float c2[6] = {c[0], 2.0f * c[1], 2.0f * c[2], c[3], 2.0f * c[4], c[5]};
            float ml[3], mh[3], R[3];
            Win w[3];
            for (int d = 0; d < 3; ++d) {
                float mn = active ? m[d] : INFINITY, mx = active ? m[d] : -INFINITY, rr = r[d];
                for (int o = kWave / 2; o > 0; o >>= 1) {
                    mn = fminf(mn, __shfl_xor(mn, o));
                    mx = fmaxf(mx, __shfl_xor(mx, o));
                    rr = fmaxf(rr, __shfl_xor(rr, o));
                }
                ml[d] = mn; mh[d] = mx; R[d] = rr;
                const HdrAx &hx = hax_of(buf);  // (an open axis: the direct image only)
                const Win wa = image_range(mn, rr, hx.ilo[d], hx.ihi[d], false);
                const Win wb = image_range(mx, rr, hx.ilo[d], hx.ihi[d], false);
                w[d].k0 = min(wa.k0, wb.k0);
                w[d].k1 = max(wa.k1, wb.k1);
            }
            for (int kz = w[2].k0; kz <= w[2].k1; ++kz)
                for (int ky = w[1].k0; ky <= w[1].k1; ++ky)
                    for (int kx = w[0].k0; kx <= w[0].k1; ++kx) {
                        const int kk[3] = {kx, ky, kz};
                        int c0[3], c1[3];
                        bool any = true;
                        for (int d = 0; d < 3; ++d) {
                            float xa, xb;
                            image_window(kk[d], R[d], xa, xb);
                            const float ta = ml[d] - xb, tb = mh[d] - xa;  // sample window
                            const float glo = h.lo[d], ghi = h.lo[d] + h.cs[d] * h.n[d];
                            if (tb < glo || ta > ghi) { any = false; break; }
                            c0[d] = cell_axis(h, d, ta);
                            c1[d] = cell_axis(h, d, tb);
                        }
                        if (!any) continue;
                        for (int cz = c0[2]; cz <= c1[2]; ++cz)
                            for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                                const int row = (cz * h.n[1] + cy) * h.n[0];
                                const int b = sstart[row + c0[0]], e = sstart[row + c1[0] + 1];
                                for (int q0 = b; q0 < e; q0 += kWave) {
                                    const int q = q0 + lane;
                                    __syncthreads();
                                    if (q < e) {
                                        const int sid = sids[q];
                                        scand[lane] = make_float4(samples[(int64_t)sid * 3], samples[(int64_t)sid * 3 + 1],
                                                                  samples[(int64_t)sid * 3 + 2], __int_as_float(sid));
                                        const float *__restrict__ hrow = hs + (int64_t)sid * SKU;
                                        if constexpr ((MASK & 1) != 0) stage_h<0>(&shrow[lane][O0], hrow + O0);
                                        if constexpr ((MASK & 2) != 0) stage_h<1>(&shrow[lane][O1], hrow + O1);
                                        if constexpr ((MASK & 4) != 0) stage_h<2>(&shrow[lane][O2], hrow + O2);
                                        if constexpr ((MASK & 8) != 0) stage_h<3>(&shrow[lane][O3], hrow + O3);
                                        if constexpr ((MASK & 16) != 0) stage_h<kFnTrace>(&shrow[lane][O4], hrow + O4);
                                        if constexpr ((MASK & 32) != 0) stage_h<kFnOp>(&shrow[lane][O5], hrow + O5);
                                    }
                                    __syncthreads();
                                    const int cnt = min(kWave, e - q0);
                                    if (active)
                                        for (int u = 0; u < cnt; ++u) {
                                            const float4 sp = scand[u];
                                            const float sv[3] = {sp.x, sp.y, sp.z};
                                            bool mine = true;
                                            for (int d = 0; d < 3; ++d) {  // inside its cut box at image kk
                                                const float x = m[d] - sv[d];
                                                mine = mine && fabsf(x - 2.0f * kk[d]) <= r[d] + 1e-5f;
                                            }
                                            if (!mine) continue;
                                            float X[3], a[3], G;
                                            if (!pair_eval(Torus{}, m, sv, c, X, G, a)) continue;
                                            const float *H = &shrow[u][0];
                                            float phi = 0.0f, gg[3] = {0.0f, 0.0f, 0.0f};
                                            float ee[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                                            if constexpr ((MASK & 1) != 0) phi_ge_add<0>(H + O0, a, c2, phi, gg, ee);
                                            if constexpr ((MASK & 2) != 0) phi_ge_add<1>(H + O1, a, c2, phi, gg, ee);
                                            if constexpr ((MASK & 4) != 0) phi_ge_add<2>(H + O2, a, c2, phi, gg, ee);
                                            if constexpr ((MASK & 8) != 0) phi_ge_add<3>(H + O3, a, c2, phi, gg, ee);
                                            if constexpr ((MASK & 16) != 0) phi_ge_add<kFnTrace>(H + O4, a, c2, phi, gg, ee);
                                            if constexpr ((MASK & 32) != 0) phi_ge_add<kFnOp>(H + O5, a, c2, phi, gg, ee, cf);
                                            vol_mom_add<TOP>(G, phi, gg, ee, X, mom);
                                        }
                                }
                            }
                    }
            float dm[3], dc[6], dv[1];
            vol_mom_finish(c, mom, dm, dc, dv);
            if (active) bwd_store<1>(g, 1, 0, 1, dm, dc, dv, dmeans, dvalues, dconics, v0);
        }
    }
}

// Big Gaussians of the fused backward: the per-function pair terms into the same sums, rows
// written once.
template <int MASK, class... CF>
__global__ __launch_bounds__(kBlock) void k_vol_backward_big_m(const char *__restrict__ buf, int P, int N,
                                                               const float *__restrict__ means,
                                                               const float *__restrict__ values,
                                                               const float *__restrict__ conics,
                                                               const float *__restrict__ samples,
                                                               const float *__restrict__ hs,
                                                               float *__restrict__ dmeans,
                                                               float *__restrict__ dvalues,
                                                               float *__restrict__ dconics, CF... coef) {
    constexpr int NV = 10, SKU = mask_ku(MASK);
    const float *cf = coef_of(coef...);
    __shared__ float part[kWavesPerBlock][NV];
    const Hdr h = hdr_of(buf);
    if (vol_stale(buf, h, P, N)) return;  // (k_vol_backward_m writes the NaN)
    const Axes ax = axes_of(buf);
    const int32_t *__restrict__ gids = reinterpret_cast<const int32_t *>(buf + h.o_gids);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    for (int b = blockIdx.x; b < h.nbig; b += gridDim.x) {
        const int g = gids[h.nsmall + b];
        float m[3], c[6];
        for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
        for (int q = 0; q < 6; ++q) c[q] = conics[(int64_t)g * 6 + q];
        const float v0 = values[g];
        float v[NV];
        for (int k = 0; k < NV; ++k) v[k] = 0.0f;
        for (int sid = threadIdx.x; sid < N; sid += kBlock) {
            const float sp[3] = {samples[(int64_t)sid * 3], samples[(int64_t)sid * 3 + 1], samples[(int64_t)sid * 3 + 2]};
            const float *hrow = hs + (int64_t)sid * SKU;
            if constexpr ((MASK & 1) != 0)
                bwd_pair<0, 1>(ax, m, c, values, g, 1, 0, 1, sp, hrow + mask_off(MASK, 0), v, v + 3, v + 9);
            if constexpr ((MASK & 2) != 0)
                bwd_pair<1, 1>(ax, m, c, values, g, 1, 0, 1, sp, hrow + mask_off(MASK, 1), v, v + 3, v + 9);
            if constexpr ((MASK & 4) != 0)
                bwd_pair<2, 1>(ax, m, c, values, g, 1, 0, 1, sp, hrow + mask_off(MASK, 2), v, v + 3, v + 9);
            if constexpr ((MASK & 8) != 0)
                bwd_pair<3, 1>(ax, m, c, values, g, 1, 0, 1, sp, hrow + mask_off(MASK, 3), v, v + 3, v + 9);
            if constexpr ((MASK & 16) != 0)
                bwd_pair<kFnTrace, 1>(ax, m, c, values, g, 1, 0, 1, sp, hrow + mask_off(MASK, kFnTrace), v, v + 3, v + 9);
            if constexpr ((MASK & 32) != 0)
                bwd_pair<kFnOp, 1>(ax, m, c, values, g, 1, 0, 1, sp, hrow + mask_off(MASK, kFnOp), v, v + 3, v + 9, cf);
        }
        for (int k = 0; k < NV; ++k)
            for (int o = kWave / 2; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
        if (lane == 0)
            for (int k = 0; k < NV; ++k) part[w][k] = v[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            float t[NV];
            for (int k = 0; k < NV; ++k) {
                t[k] = 0.0f;
                for (int q = 0; q < kWavesPerBlock; ++q) t[k] += part[q][k];
            }
            bwd_store<1>(g, 1, 0, 1, t, t + 3, t + 9, dmeans, dvalues, dconics, v0);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------ sample gradients
// dL/d samples (DESIGN.md 4.9, D = 3): per pair dL/ds = v G (phi a - A g) = -dL/dm, with phi and
// g = d phi / d a of phi_ge_t from the sample's tensor H.  The forward's walk (lane = sample,
// walk_candidates, then the big Gaussians), so the pair set is the forward's; the lane reads its
// own dL rows once, keeps H in registers, sums three values in a fixed order and stores them once.
// No atomics, no cross-lane sums, no workspace.

// the lane's H of function FN (k_vol_hsum's sums in its order, scaled as stage_h does)
template <int FN>
__device__ __forceinline__ void sg_load_h(const float *__restrict__ dL, int64_t sid, float *H) {
    constexpr int KU = VTr<FN>::KU, K = VTr<FN>::K;
    float h[KU];
    for (int u = 0; u < KU; ++u) h[u] = 0.0f;
#pragma unroll
    for (int f = 0; f < K; ++f) h[umap<FN>(f)] += dL[sid * K + f];
    for (int u = 0; u < KU; ++u) H[u] = h[u] * vol_inv_mult<FN>(u);
}
// ds += w (phi a - A g), w = v G
__device__ __forceinline__ void sg_add(float w, float phi, const float *a, const float *c, const float *g,
                                       float *ds) {
    const float Ag[3] = {c[0] * g[0] + c[1] * g[1] + c[2] * g[2], c[1] * g[0] + c[3] * g[1] + c[4] * g[2],
                         c[2] * g[0] + c[4] * g[1] + c[5] * g[2]};
    for (int d = 0; d < 3; ++d) ds[d] += w * (phi * a[d] - Ag[d]);
}

struct VDLs {
    const float *p[4];  // dL/d out per function code (fn_slot); entries outside the mask unused
};

// C = 1, every mask
template <int MASK, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_sgrad_m(const char *__restrict__ buf, int P, int N,
                                                       const float *__restrict__ means,
                                                       const float *__restrict__ values,
                                                       const float *__restrict__ conics,
                                                       const float *__restrict__ samples, VDLs dLs,
                                                       float *__restrict__ dsamples, CF... coef) {
    constexpr int SKU = mask_ku(MASK);
    constexpr int O0 = mask_off(MASK, 0), O1 = mask_off(MASK, 1), O2 = mask_off(MASK, 2), O3 = mask_off(MASK, 3);
    constexpr int O4 = mask_off(MASK, kFnTrace), S4 = fn_slot(kFnTrace);
    constexpr int O5 = mask_off(MASK, kFnOp), S5 = fn_slot(kFnOp);
    const float *cf = coef_of(coef...);
    __shared__ VCand<1> cand[kWave];
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    if (vol_stale(buf, h, P, N)) {  // stale buffer / inputs: loud
        for (int64_t i = (int64_t)blockIdx.x * kWave + lane; i < (int64_t)N * 3; i += (int64_t)gridDim.x * kWave)
            dsamples[i] = NAN;
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < h.ncells; cell += gridDim.x) {
        const int sb = bin.sstart[cell], se = bin.sstart[cell + 1];
        const int cc[3] = {cell % h.n[0], (cell / h.n[0]) % h.n[1], cell / (h.n[0] * h.n[1])};
        for (int j0 = sb; j0 < se; j0 += kWave) {
            const int j = j0 + lane;
            const bool active = j < se;
            const int sid = active ? bin.sids[j] : 0;
            float s[3], H[SKU];
            for (int d = 0; d < 3; ++d) s[d] = active ? samples[(int64_t)sid * 3 + d] : 0.0f;
            for (int u = 0; u < SKU; ++u) H[u] = 0.0f;
            if (active) {
                if constexpr ((MASK & 1) != 0) sg_load_h<0>(dLs.p[0], sid, H + O0);
                if constexpr ((MASK & 2) != 0) sg_load_h<1>(dLs.p[1], sid, H + O1);
                if constexpr ((MASK & 4) != 0) sg_load_h<2>(dLs.p[2], sid, H + O2);
                if constexpr ((MASK & 8) != 0) sg_load_h<3>(dLs.p[3], sid, H + O3);
                if constexpr ((MASK & 16) != 0) sg_load_h<kFnTrace>(dLs.p[S4], sid, H + O4);
                if constexpr ((MASK & 32) != 0) sg_load_h<kFnOp>(dLs.p[S5], sid, H + O5);
            }
            float ds[3] = {0.0f, 0.0f, 0.0f};
            auto eval = [&](const auto &ax, const float *m, const float *c, float v) {
                float X[3], a[3], G;
                if (!pair_eval(ax, m, s, c, X, G, a)) return;
                const float c2[6] = {c[0], 2.0f * c[1], 2.0f * c[2], c[3], 2.0f * c[4], c[5]};
                float phi = 0.0f, g[3] = {0.0f, 0.0f, 0.0f}, e[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // (e unused)
                if constexpr ((MASK & 1) != 0) phi_ge_add<0>(H + O0, a, c2, phi, g, e);
                if constexpr ((MASK & 2) != 0) phi_ge_add<1>(H + O1, a, c2, phi, g, e);
                if constexpr ((MASK & 4) != 0) phi_ge_add<2>(H + O2, a, c2, phi, g, e);
                if constexpr ((MASK & 8) != 0) phi_ge_add<3>(H + O3, a, c2, phi, g, e);
                if constexpr ((MASK & 16) != 0) phi_ge_add<kFnTrace>(H + O4, a, c2, phi, g, e);
                if constexpr ((MASK & 32) != 0) phi_ge_add<kFnOp>(H + O5, a, c2, phi, g, e, cf);
                sg_add(v * G, phi, a, c, g, ds);
            };
            walk_candidates<1>(
                h, hax_of(buf), bin, conics, cand, lane, cc, active, s, [&](float *vr, int g) { vr[0] = values[g]; },
                [&](const float *m, const float *c, const float *vr) { eval(Torus{}, m, c, vr[0]); });
            if (active) {
                const Axes ax = axes_of(buf);  // (the big Gaussians meet every sample: pair_eval needs the axes)
                for (int q = bin.gstart[2 * h.ncells]; q < bin.gstart[2 * h.ncells + 1]; ++q) {  // big ones
                    const int g = bin.gids[q];
                    float m[3], c[6];
                    for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
                    for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                    eval(ax, m, c, values[g]);
                }
                for (int d = 0; d < 3; ++d) dsamples[(int64_t)sid * 3 + d] = ds[d];
            }
        }
    }
}

// C > 1, one function, CB channels per launch: hv_u = sum_ch v_ch h_u,ch over the block's channels
// per pair; the launches after the first (cbase > 0) add onto the owning lane's stored row.
template <int FN, int CB, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_sgrad(const char *__restrict__ buf, int P, int N, int C, int cbase,
                                                     const float *__restrict__ means,
                                                     const float *__restrict__ values,
                                                     const float *__restrict__ conics,
                                                     const float *__restrict__ samples,
                                                     const float *__restrict__ dL, float *__restrict__ dsamples,
                                                     CF... coef) {
    constexpr int KU = VTr<FN>::KU, K = VTr<FN>::K;
    const float *cf = coef_of(coef...);
    __shared__ VCand<CB> cand[kWave];
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    const int nch = min(CB, C - cbase);
    if (vol_stale(buf, h, P, N)) {
        for (int64_t i = (int64_t)blockIdx.x * kWave + lane; i < (int64_t)N * 3; i += (int64_t)gridDim.x * kWave)
            dsamples[i] = NAN;
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < h.ncells; cell += gridDim.x) {
        const int sb = bin.sstart[cell], se = bin.sstart[cell + 1];
        const int cc[3] = {cell % h.n[0], (cell / h.n[0]) % h.n[1], cell / (h.n[0] * h.n[1])};
        for (int j0 = sb; j0 < se; j0 += kWave) {
            const int j = j0 + lane;
            const bool active = j < se;
            const int sid = active ? bin.sids[j] : 0;
            float s[3];
            for (int d = 0; d < 3; ++d) s[d] = active ? samples[(int64_t)sid * 3 + d] : 0.0f;
            float hh[KU][CB];  // the tensor H per channel of the block
            for (int u = 0; u < KU; ++u)
                for (int ch = 0; ch < CB; ++ch) hh[u][ch] = 0.0f;
            if (active) {
#pragma unroll
                for (int f = 0; f < K; ++f)
                    for (int ch = 0; ch < CB; ++ch)
                        if (ch < nch) hh[umap<FN>(f)][ch] += dL[((int64_t)sid * K + f) * C + cbase + ch];
                for (int u = 0; u < KU; ++u)
                    for (int ch = 0; ch < CB; ++ch) hh[u][ch] *= vol_inv_mult<FN>(u);
            }
            float ds[3] = {0.0f, 0.0f, 0.0f};
            auto values_of = [&](float *vr, int g) {
                for (int ch = 0; ch < CB; ++ch) vr[ch] = ch < nch ? values[(int64_t)g * C + cbase + ch] : 0.0f;
            };
            auto eval = [&](const auto &ax, const float *m, const float *c, const float *vr) {
                float X[3], a[3], G;
                if (!pair_eval(ax, m, s, c, X, G, a)) return;
                float hv[KU];
                for (int u = 0; u < KU; ++u) {
                    hv[u] = 0.0f;
                    for (int ch = 0; ch < CB; ++ch) hv[u] += vr[ch] * hh[u][ch];
                }
                const float c2[6] = {c[0], 2.0f * c[1], 2.0f * c[2], c[3], 2.0f * c[4], c[5]};
                float phi, g[3] = {0.0f, 0.0f, 0.0f}, e[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // (e unused)
                phi_ge_t<FN>(hv, a, c2, phi, g, e, cf);
                sg_add(G, phi, a, c, g, ds);
            };
            walk_candidates<CB>(h, hax_of(buf), bin, conics, cand, lane, cc, active, s, values_of,
                                [&](const float *m, const float *c, const float *vr) { eval(Torus{}, m, c, vr); });
            if (active) {
                const Axes ax = axes_of(buf);  // (the big Gaussians meet every sample: pair_eval needs the axes)
                for (int q = bin.gstart[2 * h.ncells]; q < bin.gstart[2 * h.ncells + 1]; ++q) {  // big ones
                    const int g = bin.gids[q];
                    float m[3], c[6], vr[CB];
                    for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
                    for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                    values_of(vr, g);
                    eval(ax, m, c, vr);
                }
                for (int d = 0; d < 3; ++d) {
                    float *o = dsamples + (int64_t)sid * 3 + d;
                    *o = cbase == 0 ? ds[d] : *o + ds[d];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------ C = 2..4: function masks
// Two or more of the four functions of one field of 2 <= C <= 4 channels at the same samples
// ("fused functions at C = 2..4"): one walk of the candidates and one pair_eval per
// kept pair for every function of MASK and every channel of the one block of CB = 4; the suffix
// _mc is "mask, channels".  Channels >= C of the block are selected to 0 and never loaded or stored.
template <int MASK, class F>
__host__ __device__ __forceinline__ void for_mask(F f) {  // f(integral_constant<int, FN>) per function of MASK
    if constexpr ((MASK & 1) != 0) f(std::integral_constant<int, 0>{});
    if constexpr ((MASK & 2) != 0) f(std::integral_constant<int, 1>{});
    if constexpr ((MASK & 4) != 0) f(std::integral_constant<int, 2>{});
    if constexpr ((MASK & 8) != 0) f(std::integral_constant<int, 3>{});
    if constexpr ((MASK & 16) != 0) f(std::integral_constant<int, kFnTrace>{});
    if constexpr ((MASK & 32) != 0) f(std::integral_constant<int, kFnOp>{});
}

// acc[u][ch] += v_ch G t_u for function FN with every rounding written out, so that an output does
// not depend on the other functions of the mask: fma(v, G, acc) for the gaussian and
// fma(round(v G), t_u, acc) for the others, among the staged candidates and the big Gaussians
// alike.  These are the roundings the compiler gives k_vol_forward<FN, 4>.
template <int FN, int CB>
__device__ __forceinline__ void fwd_acc_c(int nch, const float *vr, float G, const float *a, const float *c,
                                          float (*acc)[CB], const float *cf) {
    constexpr int KU = VTr<FN>::KU;
    float t[KU];
    terms<FN>(a, c, t, cf);
#pragma unroll
    for (int ch = 0; ch < CB; ++ch) {
        if (ch >= nch) continue;
        if constexpr (FN == 0) {
            acc[0][ch] = __builtin_fmaf(vr[ch], G, acc[0][ch]);
        } else {
            const float vG = rmul(vr[ch], G);
#pragma unroll
            for (int u = 0; u < KU; ++u) acc[u][ch] = __builtin_fmaf(vG, t[u], acc[u][ch]);
        }
    }
}

template <int MASK, int CB, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_forward_mc(const char *__restrict__ buf, int P, int N, int C,
                                                          const float *__restrict__ means,
                                                          const float *__restrict__ values,
                                                          const float *__restrict__ conics,
                                                          const float *__restrict__ samples, VOuts outs,
                                                          CF... coef) {
    constexpr int SKU = mask_ku(MASK);
    const float *cf = coef_of(coef...);
    __shared__ VCand<CB> cand[kWave];
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    const int nch = min(CB, C);
    if (vol_stale(buf, h, P, N)) {
        for (int64_t j = (int64_t)blockIdx.x * kWave + lane; j < N; j += (int64_t)gridDim.x * kWave)
            for_mask<MASK>([&](auto fc) {
                constexpr int FN = decltype(fc)::value, K = VTr<FN>::K;
                for (int f = 0; f < K; ++f)
                    for (int ch = 0; ch < nch; ++ch) outs.p[fn_slot(FN)][(j * K + f) * C + ch] = NAN;
            });
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < h.ncells; cell += gridDim.x) {
        const int sb = bin.sstart[cell], se = bin.sstart[cell + 1];
        const int cc[3] = {cell % h.n[0], (cell / h.n[0]) % h.n[1], cell / (h.n[0] * h.n[1])};
        for (int j0 = sb; j0 < se; j0 += kWave) {
            const int j = j0 + lane;
            const bool active = j < se;
            const int sid = active ? bin.sids[j] : 0;
            float s[3];
            for (int d = 0; d < 3; ++d) s[d] = active ? samples[(int64_t)sid * 3 + d] : 0.0f;
            float acc[SKU][CB];
            for (int u = 0; u < SKU; ++u)
                for (int ch = 0; ch < CB; ++ch) acc[u][ch] = 0.0f;
            auto values_of = [&](float *vr, int g) {
                for (int ch = 0; ch < CB; ++ch) vr[ch] = ch < nch ? values[(int64_t)g * C + ch] : 0.0f;
            };
            auto eval = [&](const auto &ax, const float *m, const float *c, const float *vr) {
                float X[3], a[3], G;
                if (!pair_eval(ax, m, s, c, X, G, a)) return;
                for_mask<MASK>([&](auto fc) {
                    constexpr int FN = decltype(fc)::value;
                    fwd_acc_c<FN, CB>(nch, vr, G, a, c, acc + mask_off(MASK, FN), cf);
                });
            };
            walk_candidates<CB>(h, hax_of(buf), bin, conics, cand, lane, cc, active, s, values_of,
                                [&](const float *m, const float *c, const float *vr) { eval(Torus{}, m, c, vr); });
            if (active) {
                const Axes ax = axes_of(buf);  // (the big Gaussians meet every sample: pair_eval needs the axes)
                for (int q = bin.gstart[2 * h.ncells]; q < bin.gstart[2 * h.ncells + 1]; ++q) {  // big ones
                    const int g = bin.gids[q];
                    float m[3], c[6], vr[CB];
                    for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
                    for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                    values_of(vr, g);
                    eval(ax, m, c, vr);
                }
                for_mask<MASK>([&](auto fc) {
                    constexpr int FN = decltype(fc)::value, K = VTr<FN>::K, O = mask_off(MASK, FN);
                    float *__restrict__ out = outs.p[fn_slot(FN)];
#pragma unroll
                    for (int f = 0; f < K; ++f)
#pragma unroll
                        for (int ch = 0; ch < CB; ++ch)
                            if (ch < nch) out[((int64_t)sid * K + f) * C + ch] = acc[O + umap<FN>(f)][ch];
                });
            }
        }
    }
}

// k_vol_hsum into function FN's slice of the concatenated rows hs[N][sum KU][C]: the slice sits at
// off = mask_off(mask, FN) * C of a row of stride = mask_ku(mask) * C floats, in k_vol_hsum's
// [KU][C] layout (bwd_pair<FN, 4> reads it unchanged).
template <int FN>
__global__ __launch_bounds__(kBlock) void k_vol_hsum_cat_c(int N, int C, const float *__restrict__ dL,
                                                           float *__restrict__ hs, int stride, int off) {
    constexpr int KU = VTr<FN>::KU, K = VTr<FN>::K;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)N * C) return;
    const int64_t sid = t / C;
    const int ch = (int)(t - sid * C);
    float h[KU];
    for (int u = 0; u < KU; ++u) h[u] = 0.0f;
#pragma unroll
    for (int f = 0; f < K; ++f) h[umap<FN>(f)] += dL[(sid * K + f) * C + ch];
    for (int u = 0; u < KU; ++u) hs[sid * stride + off + u * C + ch] = h[u];
}

// The lane = Gaussian loop nest of the backward, for k_vol_backward_mc alone (k_vol_backward and
// k_vol_backward_m keep their own copies: their contracted pair arithmetic moves with the nest,
// DESIGN.md 4.8).  The wave's Gaussians (mean m, cut half-widths r, `active` lanes) walk the image
// windows of their union; the samples of a row of cells are staged 64 at a time: stage(slot, sid)
// fills what the kernel keeps per staged sample, eval(slot, sv) takes a sample inside the lane's
// own cut box.
template <class Stage, class Eval>
__device__ __forceinline__ void walk_samples(const Hdr &h, const HdrAx &hx, const int32_t *__restrict__ sids,
                                             const int32_t *__restrict__ sstart, const float *__restrict__ samples,
                                             float4 *scand, int lane, bool active, const float *m, const float *r,
                                             Stage stage, Eval eval) {
    float ml[3], mh[3], R[3];
    Win w[3];
    for (int d = 0; d < 3; ++d) {
        float mn = active ? m[d] : INFINITY, mx = active ? m[d] : -INFINITY, rr = r[d];
        for (int o = kWave / 2; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o));
            mx = fmaxf(mx, __shfl_xor(mx, o));
            rr = fmaxf(rr, __shfl_xor(rr, o));
        }
        ml[d] = mn; mh[d] = mx; R[d] = rr;
        w[d] = box_images(hx, d, mn, mx, rr, false);
    }
    for (int kz = w[2].k0; kz <= w[2].k1; ++kz)
        for (int ky = w[1].k0; ky <= w[1].k1; ++ky)
            for (int kx = w[0].k0; kx <= w[0].k1; ++kx) {
                const int kk[3] = {kx, ky, kz};
                int c0[3], c1[3];
                bool any = true;
                for (int d = 0; d < 3 && any; ++d)  // the sample window
                    any = window_cells(h, d, kk[d], R[d], ml[d], mh[d], false, c0[d], c1[d]);
                if (!any) continue;
                for (int cz = c0[2]; cz <= c1[2]; ++cz)
                    for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                        const int row = (cz * h.n[1] + cy) * h.n[0];
                        const int b = sstart[row + c0[0]], e = sstart[row + c1[0] + 1];
                        for (int q0 = b; q0 < e; q0 += kWave) {
                            const int q = q0 + lane;
                            __syncthreads();
                            if (q < e) {
                                const int sid = sids[q];
                                scand[lane] = make_float4(samples[(int64_t)sid * 3], samples[(int64_t)sid * 3 + 1],
                                                          samples[(int64_t)sid * 3 + 2], __int_as_float(sid));
                                stage(lane, sid);
                            }
                            __syncthreads();
                            const int cnt = min(kWave, e - q0);
                            if (active)
                                for (int u = 0; u < cnt; ++u) {
                                    const float4 sp = scand[u];
                                    const float sv[3] = {sp.x, sp.y, sp.z};
                                    if (in_cut_box(m, sv, r, kk)) eval(u, sv);
                                }
                        }
                    }
            }
}

// The fused backward at C = 2..4 in the moment form (vol_mom_add / vol_mom_finish above): the lane
// keeps its v[ch]; a staged sample carries its tensors H[ch][sum KU] (hs scaled by vol_inv_mult, one
// column per channel, the columns >= C selected to 0).  Per kept pair hv_u = sum_ch v_ch H_ch,u, then
// phi, g, e of hv over the mask's functions and one vol_mom_add; dv[ch] += G phi(H_ch).  v is inside
// hv, so the rows are stored with scale 1.  No atomics, a fixed order of additions.
template <int MASK, int CB, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_backward_mc(const char *__restrict__ buf, int P, int N, int C,
                                                           const float *__restrict__ means,
                                                           const float *__restrict__ values,
                                                           const float *__restrict__ conics,
                                                           const float *__restrict__ samples,
                                                           const float *__restrict__ hs, float *__restrict__ dmeans,
                                                           float *__restrict__ dvalues, float *__restrict__ dconics,
                                                           CF... coef) {
    constexpr int SKU = mask_ku(MASK), TOP = mask_top(MASK);
    const float *cf = coef_of(coef...);
    __shared__ float4 scand[kWave];
    __shared__ float shrow[kWave][CB][SKU];  // the candidates' H, channel after channel
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    const int nch = min(CB, C);
    if (vol_stale(buf, h, P, N)) {  // stale buffer / inputs: loud
        const float nan[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
        for (int64_t i = (int64_t)blockIdx.x * kWave + lane; i < P; i += (int64_t)gridDim.x * kWave)
            bwd_store<CB>((int)i, C, 0, nch, nan, nan, nan, dmeans, dvalues, dconics);
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < 2 * h.ncells; cell += gridDim.x) {  // (class-major cells)
        const int gb = bin.gstart[cell], ge = bin.gstart[cell + 1];
        for (int i0 = gb; i0 < ge; i0 += kWave) {
            const int i = i0 + lane;
            const bool active = i < ge;
            float m[3] = {0.0f, 0.0f, 0.0f}, r[3] = {0.0f, 0.0f, 0.0f}, c[6], v[CB];
            int g = 0;
            for (int k = 0; k < 6; ++k) c[k] = 0.0f;
            for (int ch = 0; ch < CB; ++ch) v[ch] = 0.0f;
            if (active) {
                const float4 mp = bin.gpk[i], ex = bin.gek[i];
                g = __float_as_int(mp.w);
                m[0] = mp.x; m[1] = mp.y; m[2] = mp.z;
                r[0] = ex.x; r[1] = ex.y; r[2] = ex.z;
                for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                for (int ch = 0; ch < CB; ++ch)
                    if (ch < nch) v[ch] = values[(int64_t)g * C + ch];
            }
            VMom mom{};
            float dv[CB];
            for (int ch = 0; ch < CB; ++ch) dv[ch] = 0.0f;
            const float c2[6] = {c[0], 2.0f * c[1], 2.0f * c[2], c[3], 2.0f * c[4], c[5]};
            auto stage = [&](int slot, int sid) {
                const float *__restrict__ hrow = hs + (int64_t)sid * SKU * C;
                for_mask<MASK>([&](auto fc) {
                    constexpr int FN = decltype(fc)::value, KU = VTr<FN>::KU, O = mask_off(MASK, FN);
#pragma unroll
                    for (int ch = 0; ch < CB; ++ch)
#pragma unroll
                        for (int u = 0; u < KU; ++u)
                            shrow[slot][ch][O + u] = ch < nch ? hrow[(O + u) * C + ch] * vol_inv_mult<FN>(u) : 0.0f;
                });
            };
            auto eval = [&](int slot, const float *sv) {
                float X[3], a[3], G;
                if (!pair_eval(Torus{}, m, sv, c, X, G, a)) return;
                float hv[SKU];
                for (int u = 0; u < SKU; ++u) hv[u] = 0.0f;
#pragma unroll
                for (int ch = 0; ch < CB; ++ch) {
                    if (ch >= nch) continue;
                    const float *H = &shrow[slot][ch][0];
                    float p = 0.0f, gd[3] = {0.0f, 0.0f, 0.0f}, ed[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // (gd, ed unused)
                    for_mask<MASK>([&](auto fc) {
                        constexpr int FN = decltype(fc)::value;
                        phi_ge_add<FN>(H + mask_off(MASK, FN), a, c2, p, gd, ed, cf);
                    });
                    dv[ch] += G * p;
#pragma unroll
                    for (int u = 0; u < SKU; ++u) hv[u] += v[ch] * H[u];
                }
                float phi = 0.0f, gg[3] = {0.0f, 0.0f, 0.0f}, ee[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                for_mask<MASK>([&](auto fc) {
                    constexpr int FN = decltype(fc)::value;
                    phi_ge_add<FN>(hv + mask_off(MASK, FN), a, c2, phi, gg, ee, cf);
                });
                vol_mom_add<TOP>(G, phi, gg, ee, X, mom);
            };
            walk_samples(h, hax_of(buf), bin.sids, bin.sstart, samples, scand, lane, active, m, r, stage, eval);
            float dm[3], dc[6], dphi[1];
            vol_mom_finish(c, mom, dm, dc, dphi);
            if (active) bwd_store<CB>(g, C, 0, nch, dm, dc, dv, dmeans, dvalues, dconics);
        }
    }
}

// Big Gaussians of the fused backward at C = 2..4: the per-function pair terms (bwd_pair<FN, CB> on
// function FN's slice of the row) into the same block sums, rows written once.
template <int MASK, int CB, class... CF>
__global__ __launch_bounds__(kBlock) void k_vol_backward_big_mc(const char *__restrict__ buf, int P, int N, int C,
                                                                const float *__restrict__ means,
                                                                const float *__restrict__ values,
                                                                const float *__restrict__ conics,
                                                                const float *__restrict__ samples,
                                                                const float *__restrict__ hs,
                                                                float *__restrict__ dmeans,
                                                                float *__restrict__ dvalues,
                                                                float *__restrict__ dconics, CF... coef) {
    constexpr int NV = 9 + CB, SKU = mask_ku(MASK);
    const float *cf = coef_of(coef...);
    __shared__ float part[kWavesPerBlock][NV];
    const Hdr h = hdr_of(buf);
    if (vol_stale(buf, h, P, N)) return;  // (k_vol_backward_mc writes the NaN)
    const Axes ax = axes_of(buf);
    const int32_t *__restrict__ gids = reinterpret_cast<const int32_t *>(buf + h.o_gids);
    const int nch = min(CB, C);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    for (int b = blockIdx.x; b < h.nbig; b += gridDim.x) {
        const int g = gids[h.nsmall + b];
        float m[3], c[6];
        for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
        for (int q = 0; q < 6; ++q) c[q] = conics[(int64_t)g * 6 + q];
        float v[NV];
        for (int k = 0; k < NV; ++k) v[k] = 0.0f;
        for (int sid = threadIdx.x; sid < N; sid += kBlock) {
            const float sp[3] = {samples[(int64_t)sid * 3], samples[(int64_t)sid * 3 + 1], samples[(int64_t)sid * 3 + 2]};
            const float *hrow = hs + (int64_t)sid * SKU * C;
            for_mask<MASK>([&](auto fc) {
                constexpr int FN = decltype(fc)::value;
                bwd_pair<FN, CB>(ax, m, c, values, g, C, 0, nch, sp, hrow + mask_off(MASK, FN) * C, v, v + 3, v + 9, cf);
            });
        }
        for (int k = 0; k < NV; ++k)
            for (int o = kWave / 2; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
        if (lane == 0)
            for (int k = 0; k < NV; ++k) part[w][k] = v[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            float t[NV];
            for (int k = 0; k < NV; ++k) {
                t[k] = 0.0f;
                for (int q = 0; q < kWavesPerBlock; ++q) t[k] += part[q][k];
            }
            bwd_store<CB>(g, C, 0, nch, t, t + 3, t + 9, dmeans, dvalues, dconics);
        }
        __syncthreads();
    }
}

// The sample gradient of several functions at C = 2..4: k_vol_sgrad's lane (the tensor H per channel
// in registers, hv per pair) with phi and g summed over the mask's functions, as k_vol_sgrad_m does.
// Three sums per lane, one store, no cross-lane sums.
template <int MASK, int CB, class... CF>
__global__ __launch_bounds__(kWave) void k_vol_sgrad_mc(const char *__restrict__ buf, int P, int N, int C,
                                                        const float *__restrict__ means,
                                                        const float *__restrict__ values,
                                                        const float *__restrict__ conics,
                                                        const float *__restrict__ samples, VDLs dLs,
                                                        float *__restrict__ dsamples, CF... coef) {
    constexpr int SKU = mask_ku(MASK);
    const float *cf = coef_of(coef...);
    __shared__ VCand<CB> cand[kWave];
    const Hdr &h = hdr_of(buf);
    const int lane = threadIdx.x;
    const int nch = min(CB, C);
    if (vol_stale(buf, h, P, N)) {  // stale buffer / inputs: loud
        for (int64_t i = (int64_t)blockIdx.x * kWave + lane; i < (int64_t)N * 3; i += (int64_t)gridDim.x * kWave)
            dsamples[i] = NAN;
        return;
    }
    const Bin bin = bin_of(buf, h);
    for (int cell = blockIdx.x; cell < h.ncells; cell += gridDim.x) {
        const int sb = bin.sstart[cell], se = bin.sstart[cell + 1];
        const int cc[3] = {cell % h.n[0], (cell / h.n[0]) % h.n[1], cell / (h.n[0] * h.n[1])};
        for (int j0 = sb; j0 < se; j0 += kWave) {
            const int j = j0 + lane;
            const bool active = j < se;
            const int sid = active ? bin.sids[j] : 0;
            float s[3];
            for (int d = 0; d < 3; ++d) s[d] = active ? samples[(int64_t)sid * 3 + d] : 0.0f;
            float hh[SKU][CB];  // the tensors H per channel, function after function
            for (int u = 0; u < SKU; ++u)
                for (int ch = 0; ch < CB; ++ch) hh[u][ch] = 0.0f;
            if (active)
                for_mask<MASK>([&](auto fc) {
                    constexpr int FN = decltype(fc)::value, KU = VTr<FN>::KU, K = VTr<FN>::K, O = mask_off(MASK, FN);
                    const float *__restrict__ dL = dLs.p[fn_slot(FN)];
#pragma unroll
                    for (int f = 0; f < K; ++f)
#pragma unroll
                        for (int ch = 0; ch < CB; ++ch)
                            if (ch < nch) hh[O + umap<FN>(f)][ch] += dL[((int64_t)sid * K + f) * C + ch];
#pragma unroll
                    for (int u = 0; u < KU; ++u)
                        for (int ch = 0; ch < CB; ++ch) hh[O + u][ch] *= vol_inv_mult<FN>(u);
                });
            float ds[3] = {0.0f, 0.0f, 0.0f};
            auto values_of = [&](float *vr, int g) {
                for (int ch = 0; ch < CB; ++ch) vr[ch] = ch < nch ? values[(int64_t)g * C + ch] : 0.0f;
            };
            auto eval = [&](const auto &ax, const float *m, const float *c, const float *vr) {
                float X[3], a[3], G;
                if (!pair_eval(ax, m, s, c, X, G, a)) return;
                float hv[SKU];
#pragma unroll
                for (int u = 0; u < SKU; ++u) {
                    hv[u] = 0.0f;
                    for (int ch = 0; ch < CB; ++ch) hv[u] += vr[ch] * hh[u][ch];
                }
                const float c2[6] = {c[0], 2.0f * c[1], 2.0f * c[2], c[3], 2.0f * c[4], c[5]};
                float phi = 0.0f, g[3] = {0.0f, 0.0f, 0.0f}, e[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // (e unused)
                for_mask<MASK>([&](auto fc) {
                    constexpr int FN = decltype(fc)::value;
                    phi_ge_add<FN>(hv + mask_off(MASK, FN), a, c2, phi, g, e, cf);
                });
                sg_add(G, phi, a, c, g, ds);
            };
            walk_candidates<CB>(h, hax_of(buf), bin, conics, cand, lane, cc, active, s, values_of,
                                [&](const float *m, const float *c, const float *vr) { eval(Torus{}, m, c, vr); });
            if (active) {
                const Axes ax = axes_of(buf);  // (the big Gaussians meet every sample: pair_eval needs the axes)
                for (int q = bin.gstart[2 * h.ncells]; q < bin.gstart[2 * h.ncells + 1]; ++q) {  // big ones
                    const int g = bin.gids[q];
                    float m[3], c[6], vr[CB];
                    for (int d = 0; d < 3; ++d) m[d] = means[(int64_t)g * 3 + d];
                    for (int k = 0; k < 6; ++k) c[k] = conics[(int64_t)g * 6 + k];
                    values_of(vr, g);
                    eval(ax, m, c, vr);
                }
                for (int d = 0; d < 3; ++d) dsamples[(int64_t)sid * 3 + d] = ds[d];
            }
        }
    }
}

// ------------------------------------------------------------------------------ launches
struct VArgs {  // what every launch takes
    const char *buf;
    int P, N, C;
    const float *means, *values, *conics, *samples;
    hipStream_t s;
};

// The kernels' pointer structs from the caller's per-code arrays: four entries, or five / six (read
// only when the mask holds the trace / the operator, whose pointer goes into its slot).  The
// launches below take the operator's VCoef as a trailing argument and hand it on; none otherwise.
template <int MASK, class S, class T>
static S slots_of(T *const *ptrs) {
    S o;
    for (int f = 0; f < 4; ++f) o.p[f] = (MASK >> f) & 1 ? ptrs[f] : nullptr;
    if constexpr ((MASK & 16) != 0) o.p[fn_slot(kFnTrace)] = ptrs[kFnTrace];
    if constexpr ((MASK & 32) != 0) o.p[fn_slot(kFnOp)] = ptrs[kFnOp];
    return o;
}

// C = 1: every function mask
template <int MASK, class... CF>
static void launch_fwd_m(const VArgs &a, float *const *outs, const CF &...cf) {
    const VOuts o = slots_of<MASK, VOuts>(outs);
    k_vol_forward_m<MASK><<<kVolFwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.means, a.values, a.conics, a.samples, o,
                                                            cf...);
}
template <int FN>
static void launch_hsum_cat(int mask, int N, const float *const *dLs, float *hs, hipStream_t s) {
    if (!((mask >> FN) & 1)) return;
    k_vol_hsum_cat<FN><<<(unsigned)((N + kBlock - 1) / kBlock), kBlock, 0, s>>>(N, dLs[FN], hs, mask_ku(mask),
                                                                                 mask_off(mask, FN));
}
template <int MASK, class... CF>
static void launch_bwd_m(const VArgs &a, const float *const *dLs, float *hs, float *dm, float *dv, float *dc,
                         const CF &...cf) {
    launch_hsum_cat<0>(MASK, a.N, dLs, hs, a.s);
    launch_hsum_cat<1>(MASK, a.N, dLs, hs, a.s);
    launch_hsum_cat<2>(MASK, a.N, dLs, hs, a.s);
    launch_hsum_cat<3>(MASK, a.N, dLs, hs, a.s);
    launch_hsum_cat<kFnTrace>(MASK, a.N, dLs, hs, a.s);
    launch_hsum_cat<kFnOp>(MASK, a.N, dLs, hs, a.s);
    k_vol_backward_m<MASK><<<kVolBwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.means, a.values, a.conics, a.samples,
                                                             hs, dm, dv, dc, cf...);
    k_vol_backward_big_m<MASK><<<256, kBlock, 0, a.s>>>(a.buf, a.P, a.N, a.means, a.values, a.conics, a.samples, hs,
                                                        dm, dv, dc, cf...);
}

// one function, CB = 1 (the backward at C = 1), 4 (C <= 4) or 8 channels per launch
template <int FN, int CB, class... CF>
static void launch_fwd(const VArgs &a, float *out, const CF &...cf) {
    for (int cb = 0; cb < a.C; cb += CB)
        k_vol_forward<FN, CB><<<kVolFwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.C, cb, a.means, a.values, a.conics,
                                                                a.samples, out, (unsigned long long *)nullptr, cf...);
}
template <int FN, int CB, class... CF>
static void launch_bwd(const VArgs &a, const float *dL, float *hs, float *dm, float *dv, float *dc, const CF &...cf) {
    const int64_t nh = (int64_t)a.N * a.C;
    k_vol_hsum<FN><<<(unsigned)((nh + kBlock - 1) / kBlock), kBlock, 0, a.s>>>(a.N, a.C, dL, hs);
    for (int cb = 0; cb < a.C; cb += CB) {
        k_vol_backward<FN, CB><<<kVolBwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.C, cb, a.means, a.values,
                                                                 a.conics, a.samples, hs, dm, dv, dc, cf...);
        k_vol_backward_big<FN, CB><<<256, kBlock, 0, a.s>>>(a.buf, a.P, a.N, a.C, cb, a.means, a.values, a.conics,
                                                            a.samples, hs, dm, dv, dc, cf...);
    }
}

// sample gradients: every mask at C = 1; one function, 4 (C <= 4) or 8 channels per launch
template <int MASK, class... CF>
static void launch_sgrad_m(const VArgs &a, const float *const *dLs, float *ds, const CF &...cf) {
    const VDLs d = slots_of<MASK, VDLs>(dLs);
    k_vol_sgrad_m<MASK><<<kVolFwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.means, a.values, a.conics, a.samples, d, ds,
                                                          cf...);
}
template <int FN, int CB, class... CF>
static void launch_sgrad(const VArgs &a, const float *dL, float *ds, const CF &...cf) {
    for (int cb = 0; cb < a.C; cb += CB)
        k_vol_sgrad<FN, CB><<<kVolFwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.C, cb, a.means, a.values, a.conics,
                                                              a.samples, dL, ds, cf...);
}

// C = 2..4: two or more functions, the one channel block of 4
constexpr int kVolFusedCB = DGS_VOLUME_FUSED_MAX_C;
template <int MASK, class... CF>
static void launch_fwd_mc(const VArgs &a, float *const *outs, const CF &...cf) {
    const VOuts o = slots_of<MASK, VOuts>(outs);
    k_vol_forward_mc<MASK, kVolFusedCB><<<kVolFwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.C, a.means, a.values,
                                                                          a.conics, a.samples, o, cf...);
}
template <int MASK, class... CF>
static void launch_bwd_mc(const VArgs &a, const float *const *dLs, float *hs, float *dm, float *dv, float *dc,
                          const CF &...cf) {
    const int64_t nh = (int64_t)a.N * a.C;
    for_mask<MASK>([&](auto fc) {
        constexpr int FN = decltype(fc)::value;
        k_vol_hsum_cat_c<FN><<<(unsigned)((nh + kBlock - 1) / kBlock), kBlock, 0, a.s>>>(
            a.N, a.C, dLs[FN], hs, mask_ku(MASK) * a.C, mask_off(MASK, FN) * a.C);
    });
    k_vol_backward_mc<MASK, kVolFusedCB><<<kVolBwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.C, a.means, a.values,
                                                                           a.conics, a.samples, hs, dm, dv, dc,
                                                                           cf...);
    k_vol_backward_big_mc<MASK, kVolFusedCB><<<256, kBlock, 0, a.s>>>(a.buf, a.P, a.N, a.C, a.means, a.values,
                                                                      a.conics, a.samples, hs, dm, dv, dc, cf...);
}
template <int MASK, class... CF>
static void launch_sgrad_mc(const VArgs &a, const float *const *dLs, float *ds, const CF &...cf) {
    const VDLs d = slots_of<MASK, VDLs>(dLs);
    k_vol_sgrad_mc<MASK, kVolFusedCB><<<kVolFwdBlocks, kWave, 0, a.s>>>(a.buf, a.P, a.N, a.C, a.means, a.values,
                                                                        a.conics, a.samples, d, ds, cf...);
}

// the masks of the forward kernels (all 15) and of the fused backward (two or more functions)
#define DGS_VOL_MASKS_FUSED(X) X(3) X(5) X(6) X(7) X(9) X(10) X(11) X(12) X(13) X(14) X(15)
#define DGS_VOL_MASKS(X) X(1) X(2) X(4) X(8) DGS_VOL_MASKS_FUSED(X)

// the function of a single-bit mask and its channel block: case label FN * 3 + {0: CB 1, 1: CB 4, 2: CB 8}
static int fn_cb_case(int mask, int C) { return mask_top(mask) * 3 + (C <= 1 ? 0 : C <= 4 ? 1 : 2); }
#define DGS_VOL_FN_C1(X) X(0, 1) X(1, 1) X(2, 1) X(3, 1)
#define DGS_VOL_FN_CB(X) X(0, 4) X(0, 8) X(1, 4) X(1, 8) X(2, 4) X(2, 8) X(3, 4) X(3, 8)
#define DGS_VOL_FN_CB_CASE(FN, CB) FN * 3 + (CB == 1 ? 0 : CB == 4 ? 1 : 2)
// the masks with the trace (dgs_volume_*_ops): alone, and with a non-empty subset of {0, 1, 3}
#define DGS_VOL_MASKS_TRACE_FUSED(X) X(17) X(18) X(19) X(24) X(25) X(26) X(27)
#define DGS_VOL_MASKS_TRACE(X) X(16) DGS_VOL_MASKS_TRACE_FUSED(X)
// the masks with the operator (dgs_volume_*_linop): alone, and with a non-empty subset of {0, 1}
#define DGS_VOL_MASKS_OP_FUSED(X) X(33) X(34) X(35)
#define DGS_VOL_MASKS_OP(X) X(32) DGS_VOL_MASKS_OP_FUSED(X)

}  // namespace vol
}  // namespace dgs

using namespace dgs;
using namespace dgs::vol;

// Both binning entries; `who` names the caller's one in the error texts (dgs_volume_preprocess keeps its own).
static int vol_preprocess(const char *who, int periodic, int P, int N, const float *means, const float *conics,
                          const float *samples, dgs_alloc_fn alloc, void *alloc_ctx, dgs_stream_t stream, int debug) {
    const auto err = [who](int code, const char *what) { return fail(code, std::string(who) + ": " + what); };
    if (P < 0 || N < 0 || !alloc || (P > 0 && (!means || !conics)) || (N > 0 && !samples))
        return err(DGS_ERR_ARG, "bad arguments");
    if ((int64_t)P >= (1LL << 31) - 1 || (int64_t)N >= (1LL << 31) - 1)
        return err(DGS_ERR_ARG, "too many Gaussians or samples");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // cell cap: at most 128^3 cells, and no more than ~2 per point
    const int64_t cap = std::min<int64_t>((int64_t)kAxisCells * kAxisCells * kAxisCells,
                                          std::max<int64_t>(64, 2 * ((int64_t)P + N)));
    const int64_t nmax = std::max<int64_t>(std::max(P, N), 1);
    Hdr h{};
    h.magic = kVolMagic;
    h.P = P;
    h.N = N;
    h.open = ~periodic & 7;
    h.o_gext = kHdrBytes;
    h.o_gids = h.o_gext + a256((size_t)P * 16);
    h.o_sids = h.o_gids + a256((size_t)P * 4);
    h.o_gstart = h.o_sids + a256((size_t)N * 4);
    h.o_sstart = h.o_gstart + a256((size_t)(2 * cap + 2) * 4);
    h.o_gpk = h.o_sstart + a256((size_t)(cap + 2) * 4);
    h.o_gek = h.o_gpk + a256((size_t)P * 16);
    h.o_mcopy = h.o_gek + a256((size_t)P * 16);
    h.o_ccopy = h.o_mcopy + a256((size_t)P * 12);
    h.o_scopy = h.o_ccopy + a256((size_t)P * 24);
    h.o_flag = h.o_scopy + a256((size_t)N * 12);
    const size_t total = h.o_flag + 256;
    char *buf = static_cast<char *>(alloc(alloc_ctx, DGS_BUF_BINNING, total));
    if (!buf) return err(DGS_ERR_ALLOC, "binning buffer");
    size_t sort_tmp = 0;
    DGS_TRY_HIP(onesweep_pairs<uint32_t>(nullptr, sort_tmp, nullptr, nullptr, nullptr, nullptr, (size_t)nmax, 0, 24, s));
    const size_t o_keys = 256, o_keys2 = o_keys + a256(nmax * 4), o_vals = o_keys2 + a256(nmax * 4),
                 o_tmp = o_vals + a256(nmax * 4);
    char *scr = static_cast<char *>(alloc(alloc_ctx, DGS_BUF_SCRATCH, o_tmp + a256(sort_tmp)));
    if (!scr) return err(DGS_ERR_ALLOC, "scratch");
    Red *red = reinterpret_cast<Red *>(scr);
    uint32_t *keys = reinterpret_cast<uint32_t *>(scr + o_keys), *keys2 = reinterpret_cast<uint32_t *>(scr + o_keys2);
    uint32_t *vals = reinterpret_cast<uint32_t *>(scr + o_vals);
    float4 *gext = reinterpret_cast<float4 *>(buf + h.o_gext);
    k_vol_init<<<1, 64, 0, s>>>(red);
    if (P > 0) k_vol_classify<<<(unsigned)((P + kBlock - 1) / kBlock), kBlock, 0, s>>>(P, means, conics, gext, red);
    if (N > 0) k_vol_sbounds<<<(unsigned)std::min<int64_t>((N + kBlock - 1) / kBlock, 1024), kBlock, 0, s>>>(N, samples, red);
    DGS_LAUNCH_CHECK(s, debug);
    Red hr;
    DGS_TRY_HIP(hipMemcpyAsync(&hr, red, sizeof(Red), hipMemcpyDeviceToHost, s));
    DGS_TRY_HIP(hipStreamSynchronize(s));  // the one host sync: grid sizing
    h.nbig = hr.nbig;
    h.nsmall = P - hr.nbig;
    int64_t ncells = 1;
    for (int d = 0; d < 3; ++d) {
        float lo = std::min(hr.mlo[d], hr.slo[d]), hi = std::max(hr.mhi[d], hr.shi[d]);
        if (!(lo <= hi)) lo = hi = 0.0f;  // (no small Gaussian and no sample)
        if (!std::isfinite(lo) || !std::isfinite(hi)) return err(DGS_ERR_ARG, "non-finite samples");
        h.lo[d] = lo;
        h.E[d] = hr.E[d];
        const float ext = hi - lo;
        // a quarter of the largest cut: an image window then spans <= 10 cells per axis and its
        // candidate volume (2E + E/4)^3 instead of (3E)^3 at cell = E
        h.cs[d] = std::max({0.25f * hr.E[d], ext / (float)kAxisCells, 1e-6f, ext * 1e-6f});
    }
    for (int it = 0; it < 64; ++it) {
        ncells = 1;
        for (int d = 0; d < 3; ++d) {
            const float ext = std::max(hr.mhi[d], hr.shi[d]) - h.lo[d];
            const int n = (std::isfinite(ext) && ext > 0.0f) ? (int)std::floor(ext / h.cs[d]) + 1 : 1;
            h.n[d] = std::min(std::max(n, 1), kAxisCells);
            ncells *= h.n[d];
        }
        if (ncells <= cap) break;
        for (int d = 0; d < 3; ++d) h.cs[d] *= 1.26f;
    }
    // grid end lo + cs * n must cover hi: floor(ext / cs) + 1 cells do, unless capped at 128 (then
    // cs >= ext / 128 already makes 128 cells cover it)
    h.ncells = (int)ncells;
    // two reach classes: the window of a class is its own largest cut (about half the small
    // Gaussians fall in class 0 for a uniform spread of sizes)
    h.split = 0.7f * std::max({hr.E[0], hr.E[1], hr.E[2]});
    for (int d = 0; d < 3; ++d) {
        h.Ec[0][d] = std::min(hr.E[d], h.split);
        h.Ec[1][d] = hr.E[d];
    }
    unsigned bits = 1;
    while ((1ull << bits) <= (uint64_t)(2 * ncells)) ++bits;
    int32_t *gstart = reinterpret_cast<int32_t *>(buf + h.o_gstart);
    int32_t *sstart = reinterpret_cast<int32_t *>(buf + h.o_sstart);
    for (int side = 0; side < 2; ++side) {
        const int n = side == 0 ? P : N;
        const float *pts = side == 0 ? means : samples;
        int32_t *ids = reinterpret_cast<int32_t *>(buf + (side == 0 ? h.o_gids : h.o_sids));
        int32_t *start = side == 0 ? gstart : sstart;
        if (n > 0) {
            k_vol_keys<<<(unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, s>>>(n, h, pts, side == 0 ? gext : nullptr,
                                                                              keys, vals);
            size_t tb = sort_tmp;
            DGS_TRY_HIP(onesweep_pairs<uint32_t>(scr + o_tmp, tb, keys, keys2, vals, reinterpret_cast<uint32_t *>(ids),
                                                 (size_t)n, 0, bits, s));
        }
        const int64_t nthr = std::max<int64_t>(n, 1);
        k_vol_starts<<<(unsigned)((nthr + kBlock - 1) / kBlock), kBlock, 0, s>>>(
            n, side == 0 ? 2 * h.ncells : h.ncells, keys2, start);
        DGS_LAUNCH_CHECK(s, debug);
    }
    if (h.nsmall > 0)
        k_vol_pack<<<(unsigned)((h.nsmall + kBlock - 1) / kBlock), kBlock, 0, s>>>(
            h.nsmall, reinterpret_cast<const int32_t *>(buf + h.o_gids), means, gext,
            reinterpret_cast<float4 *>(buf + h.o_gpk), reinterpret_cast<float4 *>(buf + h.o_gek));
    if (P > 0) DGS_TRY_HIP(hipMemcpyAsync(buf + h.o_mcopy, means, (size_t)P * 12, hipMemcpyDeviceToDevice, s));
    if (P > 0) DGS_TRY_HIP(hipMemcpyAsync(buf + h.o_ccopy, conics, (size_t)P * 24, hipMemcpyDeviceToDevice, s));
    if (N > 0) DGS_TRY_HIP(hipMemcpyAsync(buf + h.o_scopy, samples, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
    DGS_TRY_HIP(hipMemsetAsync(buf + h.o_flag, 0, 4, s));
    HdrAx hx;
    for (int d = 0; d < 3; ++d) {
        const bool open = (h.open >> d) & 1;
        hx.ilo[d] = open ? INFINITY : h.lo[d];
        hx.ihi[d] = open ? -INFINITY : h.lo[d] + h.cs[d] * h.n[d];
        hx.lim[d] = open ? INFINITY : 1.0f;
    }
    k_vol_header<<<1, 64, 0, s>>>(h, hx, buf);
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_preprocess_axes(int periodic, int P, int N, const float *means, const float *conics,
                                          const float *samples, dgs_alloc_fn alloc, void *alloc_ctx,
                                          dgs_stream_t stream, int debug) {
    if (periodic < 0 || periodic > 7)
        return fail(DGS_ERR_ARG, "dgs_volume_preprocess_axes: periodic must be 0..7 (bit d: axis d periodic)");
    return vol_preprocess("dgs_volume_preprocess_axes", periodic, P, N, means, conics, samples, alloc, alloc_ctx, stream,
                          debug);
}

extern "C" int dgs_volume_preprocess(int P, int N, const float *means, const float *conics, const float *samples,
                                     dgs_alloc_fn alloc, void *alloc_ctx, dgs_stream_t stream, int debug) {
    return vol_preprocess("dgs_volume_preprocess", 7, P, N, means, conics, samples, alloc, alloc_ctx, stream, debug);
}

// ---- the calls (include/dgs_volume.h).  A function is the single-bit mask 1 << function; a
// function code out of range becomes mask 0, which vol_check refuses.
static int fn_mask(int function) { return function < 0 || function > 3 ? 0 : 1 << function; }

static size_t vol_workspace(int mask, int N, int C, int backward) {
    const bool one = mask == 1 || mask == 2 || mask == 4 || mask == 8;
    if (mask < 1 || mask > 15 || !backward || N <= 0 || C <= 0 || (!one && C != 1)) return 0;
    return (size_t)N * mask_ku(mask) * C * 4;  // hs[N][unique components][C]
}
extern "C" size_t dgs_volume_workspace_size(int function, int P, int N, int C, int backward) {
    return vol_workspace(fn_mask(function), N, C, backward);
}
extern "C" size_t dgs_volume_workspace_size_multi(int mask, int P, int N, int C, int backward) {
    return vol_workspace(mask, N, C, backward);
}

// multi: the call came through a *_multi entry (the messages name what that caller passed)
static int vol_check(bool multi, int mask, int P, int N, int C, const void *binning, size_t bytes) {
    if (mask < 1 || mask > 15)
        return fail(DGS_ERR_ARG, multi ? "dgs_volume_*_multi: mask must be 1..15" : "dgs_volume: function must be 0..3");
    if (P < 0 || N < 0 || C < 1) return fail(DGS_ERR_ARG, "dgs_volume: bad sizes");
    if ((mask & (mask - 1)) != 0 && C != 1)
        return fail(DGS_ERR_ARG,
                    "dgs_volume_*_multi: several functions need C = 1; call the per-function entry points and add");
    if (!binning || bytes < kHdrBytes) return fail(DGS_ERR_BUFFER, "dgs_volume: binning buffer missing or too small");
    return DGS_OK;
}

// The call-time check of k_vol_verify (the header's offsets are read on the device).
static int vol_flag_reset_verify(int P, int N, const float *means, const float *conics, const float *samples,
                                 const void *binning, hipStream_t s) {
    char *buf = static_cast<char *>(const_cast<void *>(binning));
    const int64_t n = (int64_t)P * 9 + (int64_t)N * 3;
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((n + kBlock - 1) / kBlock, 1), 2048);
    k_vol_flag_reset<<<1, 64, 0, s>>>(P, N, buf);
    k_vol_verify<<<blocks, kBlock, 0, s>>>(P, N, reinterpret_cast<const uint32_t *>(means),
                                           reinterpret_cast<const uint32_t *>(conics),
                                           reinterpret_cast<const uint32_t *>(samples), buf);
    DGS_TRY_HIP(hipGetLastError());
    return DGS_OK;
}

static int vol_forward(bool multi, int mask, int P, int N, int C, const float *means, const float *values, const float *conics,
                       const float *samples, const void *binning, size_t binning_bytes, float *const *outs,
                       dgs_stream_t stream, int debug) {
    if (int rc = vol_check(multi, mask, P, N, C, binning, binning_bytes)) return rc;
    if (!outs) return fail(DGS_ERR_ARG, "dgs_volume_forward_multi: outs required");
    if (N == 0) return DGS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    if (C == 1) {  // every mask, a single function included
        switch (mask) {
#define X(M) case M: launch_fwd_m<M>(a, outs); break;
            DGS_VOL_MASKS(X)
#undef X
        }
    } else {  // (vol_check: a single function)
        switch (fn_cb_case(mask, C)) {
#define X(FN, CB) case DGS_VOL_FN_CB_CASE(FN, CB): launch_fwd<FN, CB>(a, outs[FN]); break;
            DGS_VOL_FN_CB(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

static int vol_backward(bool multi, int mask, int P, int N, int C, const float *means, const float *values, const float *conics,
                        const float *samples, const float *const *dLs, const void *binning, size_t binning_bytes,
                        float *dm, float *dv, float *dc, void *workspace, size_t workspace_bytes,
                        dgs_stream_t stream, int debug) {
    if (int rc = vol_check(multi, mask, P, N, C, binning, binning_bytes)) return rc;
    if (!dLs) return fail(DGS_ERR_ARG, "dgs_volume_backward_multi: dL_douts required");
    if (workspace_bytes < vol_workspace(mask, N, C, 1))
        return fail(DGS_ERR_ARG, multi ? "dgs_volume_backward_multi: workspace too small"
                                       : "dgs_volume_backward: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) return DGS_OK;
    if (N == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dm, 0, (size_t)P * 12, s));
        DGS_TRY_HIP(hipMemsetAsync(dv, 0, (size_t)P * C * 4, s));
        DGS_TRY_HIP(hipMemsetAsync(dc, 0, (size_t)P * 24, s));
        return DGS_OK;
    }
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    float *hs = static_cast<float *>(workspace);
    if ((mask & (mask - 1)) != 0) {  // several functions (C = 1)
        switch (mask) {
#define X(M) case M: launch_bwd_m<M>(a, dLs, hs, dm, dv, dc); break;
            DGS_VOL_MASKS_FUSED(X)
#undef X
        }
    } else {
        switch (fn_cb_case(mask, C)) {
#define X(FN, CB) case DGS_VOL_FN_CB_CASE(FN, CB): launch_bwd<FN, CB>(a, dLs[FN], hs, dm, dv, dc); break;
            DGS_VOL_FN_C1(X) DGS_VOL_FN_CB(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_forward(int function, int P, int N, int C, const float *means, const float *values,
                                  const float *conics, const float *samples, const void *binning,
                                  size_t binning_bytes, float *out, dgs_stream_t stream, int debug) {
    float *outs[4] = {nullptr, nullptr, nullptr, nullptr};
    if (fn_mask(function)) outs[function] = out;
    return vol_forward(false, fn_mask(function), P, N, C, means, values, conics, samples, binning, binning_bytes, outs,
                       stream, debug);
}

extern "C" int dgs_volume_backward(int function, int P, int N, int C, const float *means, const float *values,
                                   const float *conics, const float *samples, const float *dL_dout,
                                   const void *binning, size_t binning_bytes, float *dL_dmeans, float *dL_dvalues,
                                   float *dL_dconics, void *workspace, size_t workspace_bytes, dgs_stream_t stream,
                                   int debug) {
    const float *dLs[4] = {nullptr, nullptr, nullptr, nullptr};
    if (fn_mask(function)) dLs[function] = dL_dout;
    return vol_backward(false, fn_mask(function), P, N, C, means, values, conics, samples, dLs, binning, binning_bytes,
                        dL_dmeans, dL_dvalues, dL_dconics, workspace, workspace_bytes, stream, debug);
}

extern "C" int dgs_volume_forward_multi(int mask, int P, int N, int C, const float *means, const float *values,
                                        const float *conics, const float *samples, const void *binning,
                                        size_t binning_bytes, float *const *outs, dgs_stream_t stream, int debug) {
    return vol_forward(true, mask, P, N, C, means, values, conics, samples, binning, binning_bytes, outs, stream, debug);
}

extern "C" int dgs_volume_backward_multi(int mask, int P, int N, int C, const float *means, const float *values,
                                         const float *conics, const float *samples, const float *const *dL_douts,
                                         const void *binning, size_t binning_bytes, float *dL_dmeans,
                                         float *dL_dvalues, float *dL_dconics, void *workspace,
                                         size_t workspace_bytes, dgs_stream_t stream, int debug) {
    return vol_backward(true, mask, P, N, C, means, values, conics, samples, dL_douts, binning, binning_bytes, dL_dmeans,
                        dL_dvalues, dL_dconics, workspace, workspace_bytes, stream, debug);
}

// The lanes keep their dL rows in registers: no workspace (the function exists so that callers
// size it the way they size the other calls').
extern "C" size_t dgs_volume_sample_grad_workspace_size(int mask, int P, int N, int C) { return 0; }

extern "C" int dgs_volume_backward_samples(int mask, int P, int N, int C, const float *means, const float *values,
                                           const float *conics, const float *samples, const float *const *dL_douts,
                                           const void *binning, size_t binning_bytes, float *dL_dsamples,
                                           void *workspace, size_t workspace_bytes, dgs_stream_t stream, int debug) {
    if (int rc = vol_check(true, mask, P, N, C, binning, binning_bytes)) return rc;
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples: dL_douts required");
    if (N == 0) return DGS_OK;
    if (!dL_dsamples) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples: dL_dsamples required");
    for (int f = 0; f < 4; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_samples: a dL_dout of the mask is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dsamples, 0, (size_t)N * 12, s));
        return DGS_OK;
    }
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    if (C == 1) {  // every mask, a single function included
        switch (mask) {
#define X(M) case M: launch_sgrad_m<M>(a, dL_douts, dL_dsamples); break;
            DGS_VOL_MASKS(X)
#undef X
        }
    } else {  // (vol_check: a single function)
        // The lane holds KU x CB floats of H next to the walk's registers.  The forward's blocks (4 for
        // C <= 4, else 8) fit up to the laplacian (6 x 8); the third's 10 x 8 would spill, so it always
        // takes 4 channels per launch (10 x 4: no scratch).
        switch (mask_top(mask) == 3 ? DGS_VOL_FN_CB_CASE(3, 4) : fn_cb_case(mask, C)) {
#define X(FN, CB) case DGS_VOL_FN_CB_CASE(FN, CB): launch_sgrad<FN, CB>(a, dL_douts[FN], dL_dsamples); break;
            X(0, 4) X(0, 8) X(1, 4) X(1, 8) X(2, 4) X(2, 8) X(3, 4)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

// ---- the *_fused entries: several functions at 2 <= C <= DGS_VOLUME_FUSED_MAX_C take the _mc
// kernels; a single-bit mask or C = 1 is the *_multi entry itself (the same check, the same
// launches); several functions above the limit are refused (the caller's fallback).
static bool fused_mc(int mask, int C) {
    return mask >= 1 && mask <= 15 && (mask & (mask - 1)) != 0 && C >= 2 && C <= DGS_VOLUME_FUSED_MAX_C;
}
// the checks of the _mc path; `forwards`: the call belongs to the *_multi entry
static int vol_check_fused(int mask, int P, int N, int C, const void *binning, size_t bytes, bool &forwards) {
    forwards = !fused_mc(mask, C);
    if (forwards) {
        if (mask >= 1 && mask <= 15 && (mask & (mask - 1)) != 0 && C > DGS_VOLUME_FUSED_MAX_C && P >= 0 && N >= 0)
            return fail(DGS_ERR_ARG, "dgs_volume_*_fused: several functions need C <= 4 (DGS_VOLUME_FUSED_MAX_C); "
                                     "call the per-function entry points and add");
        return DGS_OK;
    }
    if (P < 0 || N < 0) return fail(DGS_ERR_ARG, "dgs_volume: bad sizes");
    if (!binning || bytes < kHdrBytes) return fail(DGS_ERR_BUFFER, "dgs_volume: binning buffer missing or too small");
    return DGS_OK;
}

extern "C" size_t dgs_volume_workspace_size_fused(int mask, int P, int N, int C, int backward) {
    if (!fused_mc(mask, C)) return vol_workspace(mask, N, C, backward);
    if (!backward || N <= 0) return 0;
    return (size_t)N * mask_ku(mask) * C * 4;  // hs[N][unique components of the mask][C]
}

extern "C" int dgs_volume_forward_fused(int mask, int P, int N, int C, const float *means, const float *values,
                                        const float *conics, const float *samples, const void *binning,
                                        size_t binning_bytes, float *const *outs, dgs_stream_t stream, int debug) {
    bool forwards;
    if (int rc = vol_check_fused(mask, P, N, C, binning, binning_bytes, forwards)) return rc;
    if (forwards)
        return vol_forward(true, mask, P, N, C, means, values, conics, samples, binning, binning_bytes, outs, stream, debug);
    if (!outs) return fail(DGS_ERR_ARG, "dgs_volume_forward_fused: outs required");
    if (N == 0) return DGS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    switch (mask) {
#define X(M) case M: launch_fwd_mc<M>(a, outs); break;
        DGS_VOL_MASKS_FUSED(X)
#undef X
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_backward_fused(int mask, int P, int N, int C, const float *means, const float *values,
                                         const float *conics, const float *samples, const float *const *dL_douts,
                                         const void *binning, size_t binning_bytes, float *dL_dmeans,
                                         float *dL_dvalues, float *dL_dconics, void *workspace,
                                         size_t workspace_bytes, dgs_stream_t stream, int debug) {
    bool forwards;
    if (int rc = vol_check_fused(mask, P, N, C, binning, binning_bytes, forwards)) return rc;
    if (forwards)
        return vol_backward(true, mask, P, N, C, means, values, conics, samples, dL_douts, binning, binning_bytes,
                            dL_dmeans, dL_dvalues, dL_dconics, workspace, workspace_bytes, stream, debug);
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_fused: dL_douts required");
    if (workspace_bytes < dgs_volume_workspace_size_fused(mask, P, N, C, 1) || (N > 0 && P > 0 && !workspace))
        return fail(DGS_ERR_ARG, "dgs_volume_backward_fused: workspace missing or too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) return DGS_OK;
    if (N == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dmeans, 0, (size_t)P * 12, s));
        DGS_TRY_HIP(hipMemsetAsync(dL_dvalues, 0, (size_t)P * C * 4, s));
        DGS_TRY_HIP(hipMemsetAsync(dL_dconics, 0, (size_t)P * 24, s));
        return DGS_OK;
    }
    for (int f = 0; f < 4; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_fused: a dL_dout of the mask is NULL");
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    float *hs = static_cast<float *>(workspace);
    switch (mask) {
#define X(M) case M: launch_bwd_mc<M>(a, dL_douts, hs, dL_dmeans, dL_dvalues, dL_dconics); break;
        DGS_VOL_MASKS_FUSED(X)
#undef X
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_backward_samples_fused(int mask, int P, int N, int C, const float *means,
                                                 const float *values, const float *conics, const float *samples,
                                                 const float *const *dL_douts, const void *binning,
                                                 size_t binning_bytes, float *dL_dsamples, void *workspace,
                                                 size_t workspace_bytes, dgs_stream_t stream, int debug) {
    bool forwards;
    if (int rc = vol_check_fused(mask, P, N, C, binning, binning_bytes, forwards)) return rc;
    if (forwards)
        return dgs_volume_backward_samples(mask, P, N, C, means, values, conics, samples, dL_douts, binning,
                                           binning_bytes, dL_dsamples, workspace, workspace_bytes, stream, debug);
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_fused: dL_douts required");
    if (N == 0) return DGS_OK;
    if (!dL_dsamples) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_fused: dL_dsamples required");
    for (int f = 0; f < 4; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_fused: a dL_dout of the mask is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dsamples, 0, (size_t)N * 12, s));
        return DGS_OK;
    }
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    switch (mask) {
#define X(M) case M: launch_sgrad_mc<M>(a, dL_douts, dL_dsamples); break;
        DGS_VOL_MASKS_FUSED(X)
#undef X
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

// ---- the *_ops entries: the *_fused entries plus function 4, the trace of the laplacian (bit 4).  A
// mask below 16 is the *_fused entry itself; the trace alone runs at any C (C = 1: the mask kernels,
// C > 1: the per-function kernels in channel blocks of 4 / 8); the trace with others of {0, 1, 3}
// takes the mask kernels at C = 1 and the _mc kernels at 2 <= C <= DGS_VOLUME_FUSED_MAX_C.
static bool ops_mask_ok(int mask) { return mask >= 1 && mask <= 31 && !((mask & 4) && (mask & 16)); }
static int vol_check_ops(int mask, int P, int N, int C, const void *binning, size_t bytes) {
    if (!ops_mask_ok(mask))
        return fail(DGS_ERR_ARG, "dgs_volume_*_ops: mask must be 1..31 without both the laplacian (4) and its trace (16)");
    if (P < 0 || N < 0 || C < 1) return fail(DGS_ERR_ARG, "dgs_volume: bad sizes");
    if (mask != 16 && C > DGS_VOLUME_FUSED_MAX_C)
        return fail(DGS_ERR_ARG, "dgs_volume_*_ops: several functions need C <= 4 (DGS_VOLUME_FUSED_MAX_C); "
                                 "call them per function and add");
    if (!binning || bytes < kHdrBytes) return fail(DGS_ERR_BUFFER, "dgs_volume: binning buffer missing or too small");
    return DGS_OK;
}

extern "C" size_t dgs_volume_workspace_size_ops(int mask, int P, int N, int C, int backward) {
    if (!ops_mask_ok(mask)) return 0;
    if (mask < 16) return dgs_volume_workspace_size_fused(mask, P, N, C, backward);
    if (!backward || N <= 0 || C <= 0 || (mask != 16 && C > DGS_VOLUME_FUSED_MAX_C)) return 0;
    return (size_t)N * mask_ku(mask) * C * 4;  // hs[N][unique components of the mask][C]
}

extern "C" int dgs_volume_forward_ops(int mask, int P, int N, int C, const float *means, const float *values,
                                      const float *conics, const float *samples, const void *binning,
                                      size_t binning_bytes, float *const *outs, dgs_stream_t stream, int debug) {
    if (ops_mask_ok(mask) && mask < 16)
        return dgs_volume_forward_fused(mask, P, N, C, means, values, conics, samples, binning, binning_bytes, outs,
                                        stream, debug);
    if (int rc = vol_check_ops(mask, P, N, C, binning, binning_bytes)) return rc;
    if (!outs) return fail(DGS_ERR_ARG, "dgs_volume_forward_ops: outs required");
    if (N == 0) return DGS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    if (C == 1) {
        switch (mask) {
#define X(M) case M: launch_fwd_m<M>(a, outs); break;
            DGS_VOL_MASKS_TRACE(X)
#undef X
        }
    } else if (mask == 16) {
        if (C <= 4) launch_fwd<kFnTrace, 4>(a, outs[kFnTrace]);
        else launch_fwd<kFnTrace, 8>(a, outs[kFnTrace]);
    } else {
        switch (mask) {
#define X(M) case M: launch_fwd_mc<M>(a, outs); break;
            DGS_VOL_MASKS_TRACE_FUSED(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_backward_ops(int mask, int P, int N, int C, const float *means, const float *values,
                                       const float *conics, const float *samples, const float *const *dL_douts,
                                       const void *binning, size_t binning_bytes, float *dL_dmeans,
                                       float *dL_dvalues, float *dL_dconics, void *workspace,
                                       size_t workspace_bytes, dgs_stream_t stream, int debug) {
    if (ops_mask_ok(mask) && mask < 16)
        return dgs_volume_backward_fused(mask, P, N, C, means, values, conics, samples, dL_douts, binning,
                                         binning_bytes, dL_dmeans, dL_dvalues, dL_dconics, workspace, workspace_bytes,
                                         stream, debug);
    if (int rc = vol_check_ops(mask, P, N, C, binning, binning_bytes)) return rc;
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_ops: dL_douts required");
    if (workspace_bytes < dgs_volume_workspace_size_ops(mask, P, N, C, 1) || (N > 0 && P > 0 && !workspace))
        return fail(DGS_ERR_ARG, "dgs_volume_backward_ops: workspace missing or too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) return DGS_OK;
    if (N == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dmeans, 0, (size_t)P * 12, s));
        DGS_TRY_HIP(hipMemsetAsync(dL_dvalues, 0, (size_t)P * C * 4, s));
        DGS_TRY_HIP(hipMemsetAsync(dL_dconics, 0, (size_t)P * 24, s));
        return DGS_OK;
    }
    for (int f = 0; f < 5; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_ops: a dL_dout of the mask is NULL");
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    float *hs = static_cast<float *>(workspace);
    if (C == 1) {
        switch (mask) {
#define X(M) case M: launch_bwd_m<M>(a, dL_douts, hs, dL_dmeans, dL_dvalues, dL_dconics); break;
            DGS_VOL_MASKS_TRACE(X)
#undef X
        }
    } else if (mask == 16) {
        if (C <= 4) launch_bwd<kFnTrace, 4>(a, dL_douts[kFnTrace], hs, dL_dmeans, dL_dvalues, dL_dconics);
        else launch_bwd<kFnTrace, 8>(a, dL_douts[kFnTrace], hs, dL_dmeans, dL_dvalues, dL_dconics);
    } else {
        switch (mask) {
#define X(M) case M: launch_bwd_mc<M>(a, dL_douts, hs, dL_dmeans, dL_dvalues, dL_dconics); break;
            DGS_VOL_MASKS_TRACE_FUSED(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_backward_samples_ops(int mask, int P, int N, int C, const float *means, const float *values,
                                               const float *conics, const float *samples,
                                               const float *const *dL_douts, const void *binning,
                                               size_t binning_bytes, float *dL_dsamples, void *workspace,
                                               size_t workspace_bytes, dgs_stream_t stream, int debug) {
    if (ops_mask_ok(mask) && mask < 16)
        return dgs_volume_backward_samples_fused(mask, P, N, C, means, values, conics, samples, dL_douts, binning,
                                                 binning_bytes, dL_dsamples, workspace, workspace_bytes, stream, debug);
    if (int rc = vol_check_ops(mask, P, N, C, binning, binning_bytes)) return rc;
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_ops: dL_douts required");
    if (N == 0) return DGS_OK;
    if (!dL_dsamples) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_ops: dL_dsamples required");
    for (int f = 0; f < 5; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_ops: a dL_dout of the mask is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dsamples, 0, (size_t)N * 12, s));
        return DGS_OK;
    }
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    if (C == 1) {
        switch (mask) {
#define X(M) case M: launch_sgrad_m<M>(a, dL_douts, dL_dsamples); break;
            DGS_VOL_MASKS_TRACE(X)
#undef X
        }
    } else if (mask == 16) {
        if (C <= 4) launch_sgrad<kFnTrace, 4>(a, dL_douts[kFnTrace], dL_dsamples);
        else launch_sgrad<kFnTrace, 8>(a, dL_douts[kFnTrace], dL_dsamples);
    } else {
        switch (mask) {
#define X(M) case M: launch_sgrad_mc<M>(a, dL_douts, dL_dsamples); break;
            DGS_VOL_MASKS_TRACE_FUSED(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

// ---- the *_linop entries: the *_ops entries plus function 5, the linear operator (bit 5), whose ten
// coefficients come as a host pointer and go to the kernels by value.  A mask below 32 is the *_ops
// entry itself; the operator alone runs at any C (C = 1: the mask kernels, C > 1: the per-function
// kernels in channel blocks of 4 / 8); the operator with the gaussian and / or the derivative takes
// the mask kernels at C = 1 and the _mc kernels at 2 <= C <= DGS_VOLUME_FUSED_MAX_C.
static bool linop_mask_ok(int mask) { return mask >= 32 ? mask <= 35 : ops_mask_ok(mask); }
static int vol_check_linop(int mask, const float *coef, int P, int N, int C, const void *binning, size_t bytes,
                           VCoef &cf) {
    if (!linop_mask_ok(mask))
        return fail(DGS_ERR_ARG, "dgs_volume_*_linop: mask must be 1..63, the operator (32) only with the gaussian (1) "
                                 "and the derivative (2)");
    if (!coef) return fail(DGS_ERR_ARG, "dgs_volume_*_linop: coef (ten floats) required with the operator");
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(coef[i])) return fail(DGS_ERR_ARG, "dgs_volume_*_linop: coef must be finite");
    if (P < 0 || N < 0 || C < 1) return fail(DGS_ERR_ARG, "dgs_volume: bad sizes");
    if (mask != 32 && C > DGS_VOLUME_FUSED_MAX_C)
        return fail(DGS_ERR_ARG, "dgs_volume_*_linop: several functions need C <= 4 (DGS_VOLUME_FUSED_MAX_C); "
                                 "call them per function and add");
    if (!binning || bytes < kHdrBytes) return fail(DGS_ERR_BUFFER, "dgs_volume: binning buffer missing or too small");
    for (int i = 0; i < 10; ++i) cf.k[i] = (i == 5 || i == 6 || i == 8 ? 2.0f : 1.0f) * coef[i];  // m_u w_u
    return DGS_OK;
}

extern "C" size_t dgs_volume_workspace_size_linop(int mask, int P, int N, int C, int backward) {
    if (!linop_mask_ok(mask)) return 0;
    if (mask < 32) return dgs_volume_workspace_size_ops(mask, P, N, C, backward);
    if (!backward || N <= 0 || C <= 0 || (mask != 32 && C > DGS_VOLUME_FUSED_MAX_C)) return 0;
    return (size_t)N * mask_ku(mask) * C * 4;  // hs[N][unique components of the mask][C]
}

extern "C" int dgs_volume_forward_linop(int mask, const float *coef, int P, int N, int C, const float *means,
                                        const float *values, const float *conics, const float *samples,
                                        const void *binning, size_t binning_bytes, float *const *outs,
                                        dgs_stream_t stream, int debug) {
    if (linop_mask_ok(mask) && mask < 32)
        return dgs_volume_forward_ops(mask, P, N, C, means, values, conics, samples, binning, binning_bytes, outs,
                                      stream, debug);
    VCoef cf;
    if (int rc = vol_check_linop(mask, coef, P, N, C, binning, binning_bytes, cf)) return rc;
    if (!outs) return fail(DGS_ERR_ARG, "dgs_volume_forward_linop: outs required");
    if (N == 0) return DGS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    if (C == 1) {
        switch (mask) {
#define X(M) case M: launch_fwd_m<M>(a, outs, cf); break;
            DGS_VOL_MASKS_OP(X)
#undef X
        }
    } else if (mask == 32) {
        if (C <= 4) launch_fwd<kFnOp, 4>(a, outs[kFnOp], cf);
        else launch_fwd<kFnOp, 8>(a, outs[kFnOp], cf);
    } else {
        switch (mask) {
#define X(M) case M: launch_fwd_mc<M>(a, outs, cf); break;
            DGS_VOL_MASKS_OP_FUSED(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_backward_linop(int mask, const float *coef, int P, int N, int C, const float *means,
                                         const float *values, const float *conics, const float *samples,
                                         const float *const *dL_douts, const void *binning, size_t binning_bytes,
                                         float *dL_dmeans, float *dL_dvalues, float *dL_dconics, void *workspace,
                                         size_t workspace_bytes, dgs_stream_t stream, int debug) {
    if (linop_mask_ok(mask) && mask < 32)
        return dgs_volume_backward_ops(mask, P, N, C, means, values, conics, samples, dL_douts, binning, binning_bytes,
                                       dL_dmeans, dL_dvalues, dL_dconics, workspace, workspace_bytes, stream, debug);
    VCoef cf;
    if (int rc = vol_check_linop(mask, coef, P, N, C, binning, binning_bytes, cf)) return rc;
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_linop: dL_douts required");
    if (workspace_bytes < dgs_volume_workspace_size_linop(mask, P, N, C, 1) || (N > 0 && P > 0 && !workspace))
        return fail(DGS_ERR_ARG, "dgs_volume_backward_linop: workspace missing or too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) return DGS_OK;
    if (N == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dmeans, 0, (size_t)P * 12, s));
        DGS_TRY_HIP(hipMemsetAsync(dL_dvalues, 0, (size_t)P * C * 4, s));
        DGS_TRY_HIP(hipMemsetAsync(dL_dconics, 0, (size_t)P * 24, s));
        return DGS_OK;
    }
    for (int f = 0; f < 6; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_linop: a dL_dout of the mask is NULL");
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    float *hs = static_cast<float *>(workspace);
    if (C == 1) {
        switch (mask) {
#define X(M) case M: launch_bwd_m<M>(a, dL_douts, hs, dL_dmeans, dL_dvalues, dL_dconics, cf); break;
            DGS_VOL_MASKS_OP(X)
#undef X
        }
    } else if (mask == 32) {
        if (C <= 4) launch_bwd<kFnOp, 4>(a, dL_douts[kFnOp], hs, dL_dmeans, dL_dvalues, dL_dconics, cf);
        else launch_bwd<kFnOp, 8>(a, dL_douts[kFnOp], hs, dL_dmeans, dL_dvalues, dL_dconics, cf);
    } else {
        switch (mask) {
#define X(M) case M: launch_bwd_mc<M>(a, dL_douts, hs, dL_dmeans, dL_dvalues, dL_dconics, cf); break;
            DGS_VOL_MASKS_OP_FUSED(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_backward_samples_linop(int mask, const float *coef, int P, int N, int C,
                                                 const float *means, const float *values, const float *conics,
                                                 const float *samples, const float *const *dL_douts,
                                                 const void *binning, size_t binning_bytes, float *dL_dsamples,
                                                 void *workspace, size_t workspace_bytes, dgs_stream_t stream,
                                                 int debug) {
    if (linop_mask_ok(mask) && mask < 32)
        return dgs_volume_backward_samples_ops(mask, P, N, C, means, values, conics, samples, dL_douts, binning,
                                               binning_bytes, dL_dsamples, workspace, workspace_bytes, stream, debug);
    VCoef cf;
    if (int rc = vol_check_linop(mask, coef, P, N, C, binning, binning_bytes, cf)) return rc;
    if (!dL_douts) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_linop: dL_douts required");
    if (N == 0) return DGS_OK;
    if (!dL_dsamples) return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_linop: dL_dsamples required");
    for (int f = 0; f < 6; ++f)
        if (((mask >> f) & 1) && !dL_douts[f])
            return fail(DGS_ERR_ARG, "dgs_volume_backward_samples_linop: a dL_dout of the mask is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) {
        DGS_TRY_HIP(hipMemsetAsync(dL_dsamples, 0, (size_t)N * 12, s));
        return DGS_OK;
    }
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    const VArgs a{static_cast<const char *>(binning), P, N, C, means, values, conics, samples, s};
    if (C == 1) {
        switch (mask) {
#define X(M) case M: launch_sgrad_m<M>(a, dL_douts, dL_dsamples, cf); break;
            DGS_VOL_MASKS_OP(X)
#undef X
        }
    } else if (mask == 32) {
        if (C <= 4) launch_sgrad<kFnOp, 4>(a, dL_douts[kFnOp], dL_dsamples, cf);
        else launch_sgrad<kFnOp, 8>(a, dL_douts[kFnOp], dL_dsamples, cf);
    } else {
        switch (mask) {
#define X(M) case M: launch_sgrad_mc<M>(a, dL_douts, dL_dsamples, cf); break;
            DGS_VOL_MASKS_OP_FUSED(X)
#undef X
        }
    }
    DGS_LAUNCH_CHECK(s, debug);
    return DGS_OK;
}

extern "C" int dgs_volume_count_pairs(int P, int N, const float *means, const float *conics, const float *samples,
                                      const void *binning, size_t binning_bytes, int64_t *counts,
                                      dgs_stream_t stream) {
    if (int rc = vol_check(false, 1, P, N, 1, binning, binning_bytes)) return rc;
    if (!counts) return fail(DGS_ERR_ARG, "dgs_volume_count_pairs: counts required");
    counts[0] = counts[1] = 0;
    if (N == 0 || P == 0) return DGS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long *d = nullptr;
    note_internal_alloc();  // (a diagnostic)
    DGS_TRY_HIP(hipMallocAsync(reinterpret_cast<void **>(&d), 24, s));
    DGS_TRY_HIP(hipMemsetAsync(d, 0, 24, s));
    if (int rc = vol_flag_reset_verify(P, N, means, conics, samples, binning, s)) return rc;
    // values are not read in COUNT mode; conics stand in for the pointer
    k_vol_forward<0, 1, true><<<kVolFwdBlocks, kWave, 0, s>>>(static_cast<const char *>(binning), P, N, 1, 0, means,
                                                              conics, conics, samples, nullptr, d);
    k_vol_flag_read<<<1, 64, 0, s>>>(P, N, static_cast<const char *>(binning), d + 2);
    unsigned long long h[3] = {0, 0, 0};
    DGS_TRY_HIP(hipMemcpyAsync(h, d, 24, hipMemcpyDeviceToHost, s));
    DGS_TRY_HIP(hipFreeAsync(d, s));
    DGS_TRY_HIP(hipStreamSynchronize(s));
    if (h[2])  // (the forward / backward write NaN instead; a count has no NaN)
        return fail(DGS_ERR_BUFFER, "dgs_volume_count_pairs: inputs differ from the binned ones or stale buffer");
    counts[0] = (int64_t)h[0];
    counts[1] = (int64_t)h[1];
    return DGS_OK;
}

// ------------------------------------------------------------------------- warm-up
// A no-op launch: the first launch of any kernel of this translation unit loads its code object
// (rocprim's kernels included) onto the device; dgs_warmup does it for every unit up front.
__global__ void k_warm_volume() {}
namespace dgs {
hipError_t warm_volume(hipStream_t s) {
    k_warm_volume<<<1, 1, 0, s>>>();
    return hipGetLastError();
}
}  // namespace dgs
