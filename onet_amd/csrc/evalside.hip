// "Next" row f-3: the evaluation step either side of the path, kept on the GPU so eval
// batches are not copied to the host per image:
//   * per-frame min-max normalisation  tensor_normal_per_frame (UT:673-689, UT = utils_20231218.py)
//   * 2-class confusion counts per image (TP, FP, FN, TN) from which _acc / _miou / _target_iou /
//     _detection_rate / _false_alarm_rate (UT:100-192) and re_assign_label (UT:410-453) follow
//   * label flip (1 - pred) for the hard re-assignment of UT:429
// HBM-bound streaming reductions: one block per plane / image, wave-shuffle + LDS combine.
//   * the validation step (include/onet_hip_eval.h): counts_kernel, the confusion counts of a whole batch in one launch spread
//     over (chunks of an image, image), straight from the head's Vt, Vd or from a label map, ground truth read in its own dtype
#include <algorithm>
#include "common.hpp"
#include "../../include/onet_hip_eval.h"

using namespace onet;

__global__ __launch_bounds__(256) void normalise_per_frame_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  int HW, float spacing) {
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
    const float den = (hi - lo) + spacing;      // (max - min + np.spacing(1)) evaluated in fp32 like torch does
    for (int i = threadIdx.x; i < HW; i += 256) dst[i] = (src[i] - lo) / den;
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

extern "C" {

int onet_normalise_per_frame(const float* x, float* y, int planes, int HW, void* stream) {
    ONET_REQUIRE(x && y && planes > 0 && HW > 0, "normalise_per_frame: bad args");
    hipLaunchKernelGGL(normalise_per_frame_kernel, dim3(planes), dim3(256), 0, as_stream(stream), x, y, HW,
                       2.220446049250313e-16f);
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
