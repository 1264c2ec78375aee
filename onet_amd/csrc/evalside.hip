// "Next" row f-3: the evaluation step either side of the path, kept on the GPU so eval
// batches are not copied to the host per image:
//   * per-frame min-max normalisation  tensor_normal_per_frame (UT:673-689, UT = utils_20231218.py)
//   * 2-class confusion counts per image (TP, FP, FN, TN) from which _acc / _miou / _target_iou /
//     _detection_rate / _false_alarm_rate (UT:100-192) and re_assign_label (UT:410-453) follow
//   * label flip (1 - pred) for the hard re-assignment of UT:429
// HBM-bound streaming reductions: one block per plane / image, wave-shuffle + LDS combine.
//   * the validation step (include/onet_hip_eval.h): counts_kernel, the confusion counts of a whole batch in one launch spread
//     over (chunks of an image, image), straight from the head's Vt, Vd or from a label map, ground truth read in its own dtype
//   * the performance report's device side (include/onet_hip_verify.h): per-frame min / max of Vt, Vd and the fp64 sums and maxima
//     get_psnr (UT:457-476) is made of, per image, by a fixed partition and a fixed-order merge (no floating-point atomics); the
//     two-stage cascade's second input, the batch's flip decision read from its confusion counts by every block
#include <algorithm>
#include "common.hpp"
#include "../../include/onet_hip_eval.h"
#include "../../include/onet_hip_verify.h"

using namespace onet;

// tensor_normal_per_frame's n(v) = (v - min) / (max - min + np.spacing(1)), evaluated in fp32 like torch does: the ONE expression of
// normalise_per_frame_kernel, moments_kernel and cascade_input_kernel, so that the three give the same bits
struct FrameScale {
    float lo, den;
    __device__ __forceinline__ FrameScale(float lo_, float hi_) : lo(lo_), den((hi_ - lo_) + 2.220446049250313e-16f) {}
    __device__ __forceinline__ float operator()(float v) const { return (v - lo) / den; }
};

__global__ __launch_bounds__(256) void normalise_per_frame_kernel(const float* __restrict__ x, float* __restrict__ y, int HW) {
    __shared__ float smin[4], smax[4];
    const float* src = x + (int64_t)blockIdx.x * HW;
    float* dst = y + (int64_t)blockIdx.x * HW;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float v = src[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = lo;
        smax[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    lo = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    hi = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    const FrameScale n(lo, hi);
    for (int i = threadIdx.x; i < HW; i += 256) dst[i] = n(src[i]);
}

// counts[b] = (TP, FP, FN, TN) with positive class 1
__global__ __launch_bounds__(256) void confusion2_kernel(const int64_t* __restrict__ pred,
                                                         const int64_t* __restrict__ target,
                                                         int64_t* __restrict__ counts, int HW) {
    __shared__ int red[4][4];
    const int64_t* p = pred + (int64_t)blockIdx.x * HW;
    const int64_t* t = target + (int64_t)blockIdx.x * HW;
    int c[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < HW; i += 256) {
        const int pp = p[i] != 0, tt = t[i] != 0;
        c[(pp && tt) ? 0 : (pp && !tt) ? 1 : (!pp && tt) ? 2 : 3] += 1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int v = c[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        counts[(int64_t)blockIdx.x * 4 + threadIdx.x] =
            (int64_t)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void flip_labels_kernel(const int64_t* __restrict__ p, int64_t* __restrict__ q, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        q[i] = 1 - p[i];
}

// ---- the validation step: per-image confusion counts added into counts[b][4] = (TP, FP, FN, TN)
// N consecutive elements as one load / store: 16 bytes (two of them for N 8-byte elements), 4 for N = 4 bytes
template <typename T, int N>
struct alignas((sizeof(T) * N > 16) ? 16 : sizeof(T) * N) Pack {
    T v[N];
};
template <typename T, int N>
__device__ __forceinline__ Pack<T, N> load_pack(const T* p) {
    return *reinterpret_cast<const Pack<T, N>*>(p);
}
template <typename T, int N>
__device__ __forceinline__ void store_pack(T* p, const Pack<T, N>& v) {
    *reinterpret_cast<Pack<T, N>*>(p) = v;
}

// A label map in its own dtype: positive where != 0 (confusion2_kernel's rule)
template <typename T>
struct LabelMap {
    const T* base;
    int64_t bs;
    template <int N>
    __device__ __forceinline__ void labels(int b, int64_t i, int HW, int (&out)[N]) const {
        const Pack<T, N> v = load_pack<T, N>(base + (int64_t)b * bs + i);
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = v.v[k] != (T)0;
    }
};

// The head's scores: label (and, where asked for, S and Y) by softmax2_label (common.hpp), each V read once
struct FromScores {
    const float *Vt, *Vd;
    float* S;
    int64_t* Y;
    template <int N>
    __device__ __forceinline__ void labels(int b, int64_t i, int HW, int (&out)[N]) const {
        const int64_t o = (int64_t)b * HW + i;
        const Pack<float, N> vt = load_pack<float, N>(Vt + o), vd = load_pack<float, N>(Vd + o);
        Pack<float, N> s0, s1;
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = softmax2_label(vt.v[k], vd.v[k], s0.v[k], s1.v[k]);
        if (S) {
            store_pack<float, N>(S + ((int64_t)b * 2 + 0) * HW + i, s0);
            store_pack<float, N>(S + ((int64_t)b * 2 + 1) * HW + i, s1);
        }
        if (Y) {
            Pack<int64_t, N> y;
#pragma unroll
            for (int k = 0; k < N; ++k) y.v[k] = out[k];
            store_pack<int64_t, N>(Y + o, y);
        }
    }
};

constexpr int COUNTS_CHUNK = 1024;      // pixels of one block's step: 256 threads x 4

// grid (chunks of an image, image).  VEC: every thread takes 4 consecutive pixels with wide loads (HW % 4 == 0, aligned operands: the
// entry point decides); else 4 pixels 256 apart with scalar loads.  Per block: wave shuffles, one LDS combine, then at most four 64-bit
// integer atomic adds -- integer sums, so the counts do not depend on the order in which the blocks arrive.
template <typename PredSource, typename GtT, bool VEC>
__global__ __launch_bounds__(256) void counts_kernel(const PredSource src, const LabelMap<GtT> gt, int64_t* __restrict__ counts, int HW) {
    __shared__ int red[4 * 4];
    const int b = blockIdx.y;
    int c[4] = {0, 0, 0, 0};
    for (int64_t base = (int64_t)blockIdx.x * COUNTS_CHUNK; base < HW; base += (int64_t)gridDim.x * COUNTS_CHUNK) {
        if (VEC) {
            const int64_t i = base + threadIdx.x * 4;
            if (i < HW) {       // (HW % 4 == 0: the four are inside together)
                int p[4], t[4];
                src.template labels<4>(b, i, HW, p);
                gt.template labels<4>(b, i, HW, t);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    c[0] += p[k] & t[k];
                    c[1] += p[k] & (t[k] ^ 1);
                    c[2] += (p[k] ^ 1) & t[k];
                    c[3] += (p[k] ^ 1) & (t[k] ^ 1);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + k * 256 + threadIdx.x;
                if (i < HW) {
                    int p[1], t[1];
                    src.template labels<1>(b, i, HW, p);
                    gt.template labels<1>(b, i, HW, t);
                    c[0] += p[0] & t[0];
                    c[1] += p[0] & (t[0] ^ 1);
                    c[2] += (p[0] ^ 1) & t[0];
                    c[3] += (p[0] ^ 1) & (t[0] ^ 1);
                }
            }
        }
    }
    block_sum_256<int, 4>(c, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c[k] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(counts + (int64_t)b * 4 + k), (unsigned long long)c[k]);
    }
}

static const int LABEL_BYTES[4] = {1, 4, 8, 4};      // dtype codes 0 uint8, 1 int32, 2 int64, 3 float32

// can 4 consecutive elements of `bytes` each be taken as one aligned load from every image of a map?
static inline bool wide_ok(const void* p, int64_t bs, int bytes) {
    const int64_t a = bytes * 4 > 16 ? 16 : bytes * 4;
    return p == nullptr || ((uintptr_t)p % a == 0 && (bs * bytes) % a == 0);
}

template <typename PredSource, typename GtT>
static int launch_counts(const PredSource& src, const void* gt, int64_t gt_bs, int64_t* counts, int B, int HW, bool vec, hipStream_t st) {
    // 1024 pixels per block and step: a 512 x 512 image alone spreads over 256 blocks; a large batch of large images loops
    const int64_t cap = std::max<int64_t>(device_cu_count(), (int64_t)8 * device_cu_count() / B);
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(HW, COUNTS_CHUNK), cap), (unsigned)B);
    const LabelMap<GtT> g{static_cast<const GtT*>(gt), gt_bs};
    if (vec)
        hipLaunchKernelGGL((counts_kernel<PredSource, GtT, true>), grid, dim3(256), 0, st, src, g, counts, HW);
    else
        hipLaunchKernelGGL((counts_kernel<PredSource, GtT, false>), grid, dim3(256), 0, st, src, g, counts, HW);
    return check_launch("counts_kernel");
}

template <typename PredSource>
static int launch_counts_gt(const PredSource& src, const void* gt, int gt_dtype, int64_t gt_bs, int64_t* counts, int B, int HW, bool vec,
                            hipStream_t st) {
    switch (gt_dtype) {
        case 0: return launch_counts<PredSource, uint8_t>(src, gt, gt_bs, counts, B, HW, vec, st);
        case 1: return launch_counts<PredSource, int32_t>(src, gt, gt_bs, counts, B, HW, vec, st);
        case 2: return launch_counts<PredSource, int64_t>(src, gt, gt_bs, counts, B, HW, vec, st);
        default: return launch_counts<PredSource, float>(src, gt, gt_bs, counts, B, HW, vec, st);
    }
}

template <typename PredT>
static int launch_label_counts(const void* pred, int64_t pred_bs, const void* gt, int gt_dtype, int64_t gt_bs, int64_t* counts, int B,
                               int HW, bool vec, hipStream_t st) {
    return launch_counts_gt(LabelMap<PredT>{static_cast<const PredT*>(pred), pred_bs}, gt, gt_dtype, gt_bs, counts, B, HW, vec, st);
}

// ---- the performance report's device side (include/onet_hip_verify.h): per-frame min / max, get_psnr's sums and maxima, the
// cascade's second-stage input.  Fixed partition: block g of an image's G = frame_parts(HW) blocks takes the COUNTS_CHUNK-pixel
// chunks g, g + G, ...; partial results go to the workspace, one wave merges them in lane order: no floating-point atomics, the
// same bits in every run.
constexpr int FRAME_PARTS = 64;       // at most one wave's lanes of partial results per image
constexpr int MOMENTS = 9;            // per image: (sum v^2 on the target, sum v^2 off it, max v on it) of X, n(Vt), n(Vd)

static inline int frame_parts(int HW) { return std::min(cdiv(HW, COUNTS_CHUNK), FRAME_PARTS); }

// (min, max) pairs of NP maps over a wave
template <int NP>
__device__ __forceinline__ void wave_minmax(float (&m)[2 * NP]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            m[2 * k] = fminf(m[2 * k], __shfl_xor(m[2 * k], o, 64));
            m[2 * k + 1] = fmaxf(m[2 * k + 1], __shfl_xor(m[2 * k + 1], o, 64));
        }
    }
}

// ... and over a 256-thread block: the result in every thread (red: 4 * 2 NP floats)
template <int NP>
__device__ __forceinline__ void block_minmax_256(float (&m)[2 * NP], float* red) {
    wave_minmax<NP>(m);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) red[(threadIdx.x >> 6) * 2 * NP + k] = m[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        m[2 * k] = fminf(fminf(red[2 * k], red[2 * NP + 2 * k]), fminf(red[4 * NP + 2 * k], red[6 * NP + 2 * k]));
        m[2 * k + 1] = fmaxf(fmaxf(red[2 * k + 1], red[2 * NP + 2 * k + 1]), fmaxf(red[4 * NP + 2 * k + 1], red[6 * NP + 2 * k + 1]));
    }
}

// grid (G, image): part[b][g][4] = (min Vt, max Vt, min Vd, max Vd) of block g's chunks
template <bool VEC>
__global__ __launch_bounds__(256) void frame_minmax_kernel(const float* __restrict__ Vt, const float* __restrict__ Vd,
                                                           float* __restrict__ part, int HW) {
    __shared__ float red[4 * 4];
    const int b = blockIdx.y;
    const float *vt = Vt + (int64_t)b * HW, *vd = Vd + (int64_t)b * HW;
    float m[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int64_t base = (int64_t)blockIdx.x * COUNTS_CHUNK; base < HW; base += (int64_t)gridDim.x * COUNTS_CHUNK) {
        if (VEC) {
            const int64_t i = base + threadIdx.x * 4;
            if (i < HW) {       // (HW % 4 == 0: the four are inside together)
                const Pack<float, 4> t = load_pack<float, 4>(vt + i), d = load_pack<float, 4>(vd + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    m[0] = fminf(m[0], t.v[k]);
                    m[1] = fmaxf(m[1], t.v[k]);
                    m[2] = fminf(m[2], d.v[k]);
                    m[3] = fmaxf(m[3], d.v[k]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + k * 256 + threadIdx.x;
                if (i < HW) {
                    const float t = vt[i], d = vd[i];
                    m[0] = fminf(m[0], t);
                    m[1] = fmaxf(m[1], t);
                    m[2] = fminf(m[2], d);
                    m[3] = fmaxf(m[3], d);
                }
            }
        }
    }
    block_minmax_256<2>(m, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[((int64_t)b * gridDim.x + blockIdx.x) * 4 + k] = m[k];
    }
}

// one pixel's share of a block's partial moments: s[2 k], s[2 k + 1] the sums of source k on / off the target, mx[k] its maximum on it
__device__ __forceinline__ void moments_add(double (&s)[6], float (&mx)[3], int t, float x, float a, float d) {
    const float v[3] = {x, a, d};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double sq = (double)v[k] * (double)v[k];
        s[2 * k] += t ? sq : 0.0;
        s[2 * k + 1] += t ? 0.0 : sq;
        mx[k] = t ? fmaxf(mx[k], v[k]) : mx[k];
    }
}

// grid (G, image), G frame_minmax_kernel's: every block merges the image's G min / max partials (block 0 stores them to minmax[b]),
// then part[b][g][9] = the moments of its chunks
template <typename GtT, bool VEC>
__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ X, int64_t x_bs, const float* __restrict__ Vt,
                                                      const float* __restrict__ Vd, const LabelMap<GtT> gt,
                                                      const float* __restrict__ mm_part, float* __restrict__ minmax,
                                                      double* __restrict__ part, int HW) {
    __shared__ float smm[4];
    __shared__ double red[4 * 6];
    __shared__ float redx[4 * 3];
    const int b = blockIdx.y, G = gridDim.x;
    if (threadIdx.x < 64) {
        float m[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
        if ((int)threadIdx.x < G) {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = mm_part[((int64_t)b * G + threadIdx.x) * 4 + k];
        }
        wave_minmax<2>(m);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                smm[k] = m[k];
                if (blockIdx.x == 0) minmax[(int64_t)b * 4 + k] = m[k];
            }
        }
    }
    __syncthreads();
    const FrameScale nt(smm[0], smm[1]), nd(smm[2], smm[3]);
    const float *x = X ? X + (int64_t)b * x_bs : nullptr, *vt = Vt + (int64_t)b * HW, *vd = Vd + (int64_t)b * HW;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float mx[3] = {0.f, 0.f, 0.f};
    for (int64_t base = (int64_t)blockIdx.x * COUNTS_CHUNK; base < HW; base += (int64_t)gridDim.x * COUNTS_CHUNK) {
        if (VEC) {
            const int64_t i = base + threadIdx.x * 4;
            if (i < HW) {
                int t[4];
                gt.template labels<4>(b, i, HW, t);
                const Pack<float, 4> pt = load_pack<float, 4>(vt + i), pd = load_pack<float, 4>(vd + i);
                Pack<float, 4> px = {{0.f, 0.f, 0.f, 0.f}};
                if (x) px = load_pack<float, 4>(x + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) moments_add(s, mx, t[k], px.v[k], nt(pt.v[k]), nd(pd.v[k]));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + k * 256 + threadIdx.x;
                if (i < HW) {
                    int t[1];
                    gt.template labels<1>(b, i, HW, t);
                    moments_add(s, mx, t[0], x ? x[i] : 0.f, nt(vt[i]), nd(vd[i]));
                }
            }
        }
    }
    block_sum_256<double, 6>(s, red);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o, 64));
        if ((threadIdx.x & 63) == 0) redx[(threadIdx.x >> 6) * 3 + k] = mx[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = part + ((int64_t)b * G + blockIdx.x) * MOMENTS;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dst[3 * k] = s[2 * k];
            dst[3 * k + 1] = s[2 * k + 1];
            dst[3 * k + 2] = (double)fmaxf(fmaxf(redx[k], redx[3 + k]), fmaxf(redx[6 + k], redx[9 + k]));
        }
    }
}

// grid (image), one wave: lane g holds block g's partial row (zeros past G), merged by wave_sum's fixed tree
__global__ __launch_bounds__(64) void moments_merge_kernel(const double* __restrict__ part, double* __restrict__ moments, int G) {
    const int b = blockIdx.x;
    double v[MOMENTS];
#pragma unroll
    for (int k = 0; k < MOMENTS; ++k) v[k] = (int)threadIdx.x < G ? part[((int64_t)b * G + threadIdx.x) * MOMENTS + k] : 0.0;
#pragma unroll
    for (int k = 0; k < MOMENTS; ++k) {
        if (k % 3 == 2) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] = fmax(v[k], __shfl_xor(v[k], o, 64));
        } else {
            v[k] = wave_sum(v[k]);
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MOMENTS; ++k) moments[(int64_t)b * MOMENTS + k] = v[k];
    }
}

// grid (blocks of an image, image); minmax == NULL: ONE block per image (the entry point's grid), which finds the selected frame's
// min / max itself.  Every block sums the batch's counts: flip = right < wrong, integers.
template <bool VEC>
__global__ __launch_bounds__(256) void cascade_input_kernel(const float* __restrict__ Vt, const float* __restrict__ Vd,
                                                            const float* __restrict__ minmax, const int64_t* __restrict__ counts,
                                                            float* __restrict__ X2, int B, int HW) {
    __shared__ long long redc[4 * 2];
    __shared__ float red[4 * 2];
    __shared__ int sflip;
    const int b = blockIdx.y;
    long long c[2] = {0, 0};      // (right, wrong) = (TP + TN, FP + FN) over the batch
    for (int i = threadIdx.x; i < B; i += 256) {
        c[0] += counts[(int64_t)i * 4 + 0] + counts[(int64_t)i * 4 + 3];
        c[1] += counts[(int64_t)i * 4 + 1] + counts[(int64_t)i * 4 + 2];
    }
    block_sum_256<long long, 2>(c, redc);
    if (threadIdx.x == 0) sflip = c[0] < c[1];
    __syncthreads();
    const bool flip = sflip != 0;
    const float* src = (flip ? Vt : Vd) + (int64_t)b * HW;
    float* dst = X2 + (int64_t)b * HW;
    float m[2] = {INFINITY, -INFINITY};
    if (minmax) {
        m[0] = minmax[(int64_t)b * 4 + (flip ? 0 : 2)];
        m[1] = minmax[(int64_t)b * 4 + (flip ? 1 : 3)];
    } else {
        for (int i = threadIdx.x; i < HW; i += 256) {
            const float v = src[i];
            m[0] = fminf(m[0], v);
            m[1] = fmaxf(m[1], v);
        }
        block_minmax_256<1>(m, red);
    }
    const FrameScale n(m[0], m[1]);
    for (int64_t base = (int64_t)blockIdx.x * COUNTS_CHUNK; base < HW; base += (int64_t)gridDim.x * COUNTS_CHUNK) {
        if (VEC) {
            const int64_t i = base + threadIdx.x * 4;
            if (i < HW) {
                Pack<float, 4> v = load_pack<float, 4>(src + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) v.v[k] = n(v.v[k]);
                store_pack<float, 4>(dst + i, v);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + k * 256 + threadIdx.x;
                if (i < HW) dst[i] = n(src[i]);
            }
        }
    }
}

template <typename GtT>
static int launch_moments(const float* X, int64_t x_bs, const float* Vt, const float* Vd, const void* gt, int64_t gt_bs,
                          const float* mm_part, float* minmax, double* part, int B, int HW, bool vec, hipStream_t st) {
    const dim3 grid((unsigned)frame_parts(HW), (unsigned)B);
    const LabelMap<GtT> g{static_cast<const GtT*>(gt), gt_bs};
    if (vec)
        hipLaunchKernelGGL((moments_kernel<GtT, true>), grid, dim3(256), 0, st, X, x_bs, Vt, Vd, g, mm_part, minmax, part, HW);
    else
        hipLaunchKernelGGL((moments_kernel<GtT, false>), grid, dim3(256), 0, st, X, x_bs, Vt, Vd, g, mm_part, minmax, part, HW);
    return check_launch("moments_kernel");
}

extern "C" {

int onet_snr_moments(const float* X, int64_t x_bs, const float* Vt, const float* Vd, const void* gt, int gt_dtype, int64_t gt_bs,
                     double* moments, float* minmax, int B, int HW, void* ws, int64_t ws_bytes, void* stream) {
    ONET_REQUIRE(Vt && Vd && gt && moments && minmax && ws, "snr_moments: null pointer");
    ONET_REQUIRE(B > 0 && B <= 65535 && HW > 0, "snr_moments: bad shape");
    ONET_REQUIRE(gt_dtype >= 0 && gt_dtype <= 3, "snr_moments: unknown dtype code %d", gt_dtype);
    ONET_REQUIRE(gt_bs >= HW && (!X || x_bs >= HW), "snr_moments: batch stride %lld / %lld below HW = %d", (long long)gt_bs,
                 (long long)x_bs, HW);
    const int64_t need = (int64_t)B * FRAME_PARTS * (MOMENTS * 8 + 4 * 4);
    ONET_REQUIRE((uintptr_t)ws % 8 == 0 && ws_bytes >= need, "snr_moments: workspace of %lld bytes (8-byte aligned) needed, %lld given",
                 (long long)need, (long long)ws_bytes);
    const hipStream_t st = as_stream(stream);
    const int G = frame_parts(HW);
    double* part = static_cast<double*>(ws);                                                            // [B][G][9]
    float* mm_part = reinterpret_cast<float*>(static_cast<char*>(ws) + (int64_t)B * FRAME_PARTS * MOMENTS * 8);   // [B][G][4]
    const bool vec_v = HW % 4 == 0 && wide_ok(Vt, HW, 4) && wide_ok(Vd, HW, 4);
    const bool vec = vec_v && wide_ok(X, x_bs, 4) && wide_ok(gt, gt_bs, LABEL_BYTES[gt_dtype]);
    const dim3 grid((unsigned)G, (unsigned)B);
    if (vec_v)
        hipLaunchKernelGGL((frame_minmax_kernel<true>), grid, dim3(256), 0, st, Vt, Vd, mm_part, HW);
    else
        hipLaunchKernelGGL((frame_minmax_kernel<false>), grid, dim3(256), 0, st, Vt, Vd, mm_part, HW);
    int rc = check_launch("frame_minmax_kernel");
    if (rc != 0) return rc;
    switch (gt_dtype) {
        case 0: rc = launch_moments<uint8_t>(X, x_bs, Vt, Vd, gt, gt_bs, mm_part, minmax, part, B, HW, vec, st); break;
        case 1: rc = launch_moments<int32_t>(X, x_bs, Vt, Vd, gt, gt_bs, mm_part, minmax, part, B, HW, vec, st); break;
        case 2: rc = launch_moments<int64_t>(X, x_bs, Vt, Vd, gt, gt_bs, mm_part, minmax, part, B, HW, vec, st); break;
        default: rc = launch_moments<float>(X, x_bs, Vt, Vd, gt, gt_bs, mm_part, minmax, part, B, HW, vec, st); break;
    }
    if (rc != 0) return rc;
    hipLaunchKernelGGL(moments_merge_kernel, dim3(B), dim3(64), 0, st, part, moments, G);
    return check_launch("moments_merge_kernel");
}

int onet_cascade_input(const float* Vt, const float* Vd, const float* minmax, const int64_t* counts, float* X2, int B, int HW,
                       void* stream) {
    ONET_REQUIRE(Vt && Vd && counts && X2, "cascade_input: null pointer");
    ONET_REQUIRE(B > 0 && B <= 65535 && HW > 0, "cascade_input: bad shape");
    const bool vec = HW % 4 == 0 && wide_ok(Vt, HW, 4) && wide_ok(Vd, HW, 4) && wide_ok(X2, HW, 4);
    // (without minmax a block scans its whole frame first: one block per image)
    const dim3 grid(minmax ? (unsigned)frame_parts(HW) : 1u, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL((cascade_input_kernel<true>), grid, dim3(256), 0, as_stream(stream), Vt, Vd, minmax, counts, X2, B, HW);
    else
        hipLaunchKernelGGL((cascade_input_kernel<false>), grid, dim3(256), 0, as_stream(stream), Vt, Vd, minmax, counts, X2, B, HW);
    return check_launch("cascade_input_kernel");
}

int onet_normalise_per_frame(const float* x, float* y, int planes, int HW, void* stream) {
    ONET_REQUIRE(x && y && planes > 0 && HW > 0, "normalise_per_frame: bad args");
    hipLaunchKernelGGL(normalise_per_frame_kernel, dim3(planes), dim3(256), 0, as_stream(stream), x, y, HW);
    return check_launch("normalise_per_frame_kernel");
}

int onet_confusion2(const int64_t* pred, const int64_t* target, int64_t* counts, int B, int HW, void* stream) {
    ONET_REQUIRE(pred && target && counts && B > 0 && HW > 0, "confusion2: bad args");
    hipLaunchKernelGGL(confusion2_kernel, dim3(B), dim3(256), 0, as_stream(stream), pred, target, counts, HW);
    return check_launch("confusion2_kernel");
}

int onet_flip_labels(const int64_t* pred, int64_t* out, int64_t n, void* stream) {
    ONET_REQUIRE(pred && out && n > 0, "flip_labels: bad args");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(flip_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), pred, out, n);
    return check_launch("flip_labels_kernel");
}

int onet_score_counts(const float* Vt, const float* Vd, const void* gt, int gt_dtype, int64_t gt_bs, float* S, int64_t* Y, int64_t* counts,
                      int B, int HW, void* stream) {
    ONET_REQUIRE(Vt && Vd && gt && counts, "score_counts: null pointer");
    ONET_REQUIRE(B > 0 && B <= 65535 && HW > 0, "score_counts: bad shape");
    ONET_REQUIRE(gt_dtype >= 0 && gt_dtype <= 3, "score_counts: unknown dtype code %d", gt_dtype);
    ONET_REQUIRE(gt_bs >= HW, "score_counts: batch stride %lld below HW = %d", (long long)gt_bs, HW);
    const bool vec = HW % 4 == 0 && wide_ok(Vt, HW, 4) && wide_ok(Vd, HW, 4) && wide_ok(S, HW, 4) && wide_ok(Y, HW, 8) &&
                     wide_ok(gt, gt_bs, LABEL_BYTES[gt_dtype]);
    return launch_counts_gt(FromScores{Vt, Vd, S, Y}, gt, gt_dtype, gt_bs, counts, B, HW, vec, as_stream(stream));
}

int onet_label_counts(const void* pred, int pred_dtype, int64_t pred_bs, const void* gt, int gt_dtype, int64_t gt_bs, int64_t* counts,
                      int B, int HW, void* stream) {
    ONET_REQUIRE(pred && gt && counts, "label_counts: null pointer");
    ONET_REQUIRE(B > 0 && B <= 65535 && HW > 0, "label_counts: bad shape");
    ONET_REQUIRE(pred_dtype >= 0 && pred_dtype <= 3 && gt_dtype >= 0 && gt_dtype <= 3, "label_counts: unknown dtype code %d / %d",
                 pred_dtype, gt_dtype);
    ONET_REQUIRE(pred_bs >= HW && gt_bs >= HW, "label_counts: batch stride %lld / %lld below HW = %d", (long long)pred_bs,
                 (long long)gt_bs, HW);
    const bool vec = HW % 4 == 0 && wide_ok(pred, pred_bs, LABEL_BYTES[pred_dtype]) && wide_ok(gt, gt_bs, LABEL_BYTES[gt_dtype]);
    const hipStream_t st = as_stream(stream);
    switch (pred_dtype) {
        case 0: return launch_label_counts<uint8_t>(pred, pred_bs, gt, gt_dtype, gt_bs, counts, B, HW, vec, st);
        case 1: return launch_label_counts<int32_t>(pred, pred_bs, gt, gt_dtype, gt_bs, counts, B, HW, vec, st);
        case 2: return launch_label_counts<int64_t>(pred, pred_bs, gt, gt_dtype, gt_bs, counts, B, HW, vec, st);
        default: return launch_label_counts<float>(pred, pred_bs, gt, gt_dtype, gt_bs, counts, B, HW, vec, st);
    }
}

}  // extern "C"
