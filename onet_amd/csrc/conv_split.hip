// 3x3 convolution forward + dgrad with fp32 tensors and fp32-LEVEL accuracy on the bf16 matrix cores, by OPERAND SPLITTING
// (F.conv2d / its input gradient at OV:47,51; the default fp32 algorithm of round 3 wherever the map is at least 32 pixels wide).
//
//   x = x_hi + x_mid + (x_lo),  w = w_hi + w_mid + (w_lo)   with every part a bf16 number (x_hi = bf16(x), x_mid = bf16(x - x_hi)):
//   hi + mid carry 16 significant bits, and   x * w  ~=  x_hi w_hi + x_hi w_mid + x_mid w_hi   drops only terms of relative size
//   2^-16 (mid * mid, hi * lo).  Each product of two bf16 numbers is exact in the fp32 accumulator of
//   v_mfma_f32_32x32x16_bf16, so the convolution costs THREE bf16 MFMAs per (tap, 16 channels) at 16x the fp32 MFMA rate:
//   5.3x the fp32 matrix peak, against 4x (x 0.5-0.6 pipe occupancy) for the fp32 Winograd F(4x4,3x3) kernel it replaces.
//   Measured against fp64 at Cin = 512: 9.7e-7 rms / 4.4e-6 max of the output scale from the split itself
//   (emulated on the CPU; F(4x4): 2.7e-6 / 4e-5), plus the fp32 accumulation of the MFMA chain as in every other kernel here.
//
// Structure: a direct implicit GEMM (M = output channels, N = 32 consecutive pixels of an image row,
// K = 16 input channels per MFMA; LDS tiles made of 16-byte slots of 8 channels, the two 8-channel halves apart; persistent
// blocks whose load -> LDS -> MFMA pipeline runs across tile boundaries), with:
//  * both parts of both operands in LDS: weights [part][tap][half][co], input halo tile [part][half][pixel] -- the fp32
//    input is loaded ONCE per chunk (8 channel planes per slot, coalesced along x) and split on the way into LDS (2 x 8
//    v_cvt_pk_bf16_f32 + 8 v_sub per slot); the weights are split once per optimizer step by the pack kernel;
//  * 8 waves per block (one block per CU, two waves per SIMD: the doubled tiles need 156 KB of LDS): 64 output channels x 16
//    image rows x 32 pixels, 2 rows per wave; per 16-channel chunk a wave issues 60 ds_read_b128 for 108 MFMAs of 32 cycles,
//    and the block moves 39 KB of input + 36 KB of weights per 864 MFMAs -- a third of the bytes and requests per
//    MFMA of the round-2 bf16 kernel this structure came from, which is what bound that kernel (DESIGN_HISTORY.md 4.2d).
// Requires Cin % 16 == 0 and W > 16; everything else takes the fp32 Winograd / direct kernels.
#include <algorithm>
#include <cstdlib>
#include "common.hpp"
#include "../../include/onet_hip_ragged.h"
#include "../../include/onet_hip_ragged_split.h"
#include "../../include/onet_hip_anymap.h"
#include "../../include/onet_hip_pairs.h"
#include "../../include/onet_hip_split_pairs.h"

using namespace onet;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));
typedef float f32x4s __attribute__((ext_vector_type(4)));

namespace {

constexpr unsigned OOB_S = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t s_rsrc(const void* base, int64_t bytes) {
    const int n = bytes > 0x7fffffffll ? 0x7fffffff : (int)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}
// (hi, mid) parts of two fp32 values, packed: hi = bf16(v) (round to nearest even), mid = bf16(v - hi)
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& mid) {
    const bf16x2 h = {(__bf16)a, (__bf16)b};
    const bf16x2 m = {(__bf16)(a - (float)h[0]), (__bf16)(b - (float)h[1])};
    hi = __builtin_bit_cast(unsigned, h);
    mid = __builtin_bit_cast(unsigned, m);
}

// The FORWARD convolution splits into fp16 parts instead (F16): hi = fp16(v), mid = fp16(v - hi) carry 22 significant bits where
// the bf16 pair carries 16, at the same three MFMAs per term (v_mfma_f32_32x32x16_f16, same rate) -- the forward error drops from
// 8e-7 rms of the output scale to the fp32 direct kernel's level, which is what the saturated B = 32 gradient check needed (the
// forward kernel alone put it at 3.3e-4; input and weight gradients contribute nothing measurable).  fp16's range is the price:
// activations (BatchNorm outputs, |x| << 65504) fit as they are, weights are packed times 2^8 so that their mid parts stay normal
// numbers (undone on the accumulators, exactly); gradients -- whose magnitude is anyone's guess -- keep the bf16 split.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {       // two bf16 (round to nearest even) in one dword, `lo` first
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void split2h(float a, float b, unsigned& hi, unsigned& mid) {
    const f16x2 h = {(_Float16)a, (_Float16)b};
    const f16x2 m = {(_Float16)(a - (float)h[0]), (_Float16)(b - (float)h[1])};
    hi = __builtin_bit_cast(unsigned, h);
    mid = __builtin_bit_cast(unsigned, m);
}

__global__ void absmax_slots_kernel(const float* __restrict__ v, int64_t n, unsigned* __restrict__ slots) {
    float m = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(v[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0)
        atomicMax(slots + ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (AMAX_SLOTS - 1)) * AMAX_STRIDE, __builtin_bit_cast(unsigned, m));
}

// w [Cout][Cin][3][3] fp32 -> wq [K/16][part 2][9][2][N][8] bf16: chunk of 16 reduction channels, part (hi, mid), tap,
// 8-channel half, output channel, channel within the half.  which = 0: forward (K = Cin, N = Cout); 1: input gradient
// (K = Cout rounded up to 16 with a zero tail, N = Cin, taps rotated by 180 degrees).
// f16: fp16 parts of s w with s = 2^k chosen from the tensor's largest magnitude (wamax slots; amax lands in [2^13, 2^14): the mid
// parts stay normal numbers down to 2^-27 of the largest weight, and no weight overflows whatever a loaded checkpoint holds);
// the two floats (s, 1 / s) are stored BEHIND the pack (element offset 2 K 9 N) for the convolution to undo s on its accumulators.
// f16 == 2: ONE part, bf16(w) (BASELINE configs[2]: plain bf16 operands), same slot order -- [K/16][9][2][N][8], i.e. two consecutive
// 16-channel chunks look exactly like the (hi | mid) pair of the split packs, which is how the 32-channel chunks of the plain-bf16
// kernels read them.
__global__ void pack3x3_split_kernel(const float* __restrict__ w, __bf16* __restrict__ wq, int Cout, int Cin, int which, int f16,
                                     const unsigned* __restrict__ wamax) {
    const int K = which == 0 ? Cin : ((Cout + 15) / 16) * 16, N = which == 0 ? Cout : Cin;
    const int64_t n = (int64_t)K * 9 * N;                            // elements of ONE part
    const int nparts = f16 == 2 ? 1 : 2;
    float winv = 1.f;
    const float wscale = f16 == 1 ? amax_scale(amax_read(wamax), true, winv) : 1.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float* meta = reinterpret_cast<float*>(wq + nparts * n);
        meta[0] = wscale;
        meta[1] = winv;
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int kc = (int)(i & 7);
        int64_t r = i >> 3;
        const int nn = (int)(r % N);
        r /= N;
        const int half = (int)(r & 1);
        r >>= 1;
        const int t = (int)(r % 9), kg = (int)(r / 9);
        const int k = kg * 16 + half * 8 + kc;
        float v = 0.f;
        if (which == 0) v = w[((int64_t)nn * Cin + k) * 9 + t];
        else if (k < Cout) v = w[((int64_t)k * Cin + nn) * 9 + (8 - t)];
        const int64_t per_chunk_part = (int64_t)9 * 2 * N * 8;
        const int64_t within = i - (int64_t)kg * per_chunk_part;     // [tap][half][n][8] inside the chunk
        if (f16 == 2) {
            wq[(int64_t)kg * per_chunk_part + within] = (__bf16)v;
        } else if (f16) {                                            // fp16 parts of 2^k w
            _Float16* wh = reinterpret_cast<_Float16*>(wq);
            const float vs = v * wscale;
            const _Float16 hi = (_Float16)vs;
            wh[((int64_t)kg * 2 + 0) * per_chunk_part + within] = hi;
            wh[((int64_t)kg * 2 + 1) * per_chunk_part + within] = (_Float16)(vs - (float)hi);
        } else {
            const __bf16 hi = (__bf16)v;
            wq[((int64_t)kg * 2 + 0) * per_chunk_part + within] = hi;
            wq[((int64_t)kg * 2 + 1) * per_chunk_part + within] = (__bf16)(v - (float)hi);
        }
    }
}

struct SpArgs {
    const float* x;       // fp32 NCHW
    int64_t x_bs;
    const __bf16* wq;     // [Cin/16][2][9][2][Cout][8]
    float* z;
    int64_t z_bs;
    int B, Cin, Cout, H, W, tilesX, tilesY, coTiles;
    float* stats;         // ST: BatchNorm partials [Cout][B * tilesY * tilesX][3] = (n, mean, M2) per tile
    const float* nsave;   // NORM: x is the PRE-activation of the Conv-BatchNorm-ReLU unit below; its coefficients [groups][4][Cin]
    int nimg;             //       (rows mean, invstd, scale, shift; bn.hip) for statistics groups of nimg consecutive images
    const unsigned* x_amax;   // F16: magnitude slots of x (NULL: no scaling)
    int x_always;             //      1: scale x so that its amax lands in [2^13, 2^14) (gradients); 0: only as an overflow guard
};

// sum over the 32 lanes of a wave half, valid in lanes 31 / 63 (DPP row rotations + row broadcast)
#define ONET_SP_DPP_ADD(v, ctrl, rmask) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, false))
__device__ __forceinline__ float sp_half_sum(float v) {
    ONET_SP_DPP_ADD(v, 0x128, 0xf);   // row_ror:8
    ONET_SP_DPP_ADD(v, 0x124, 0xf);   // row_ror:4
    ONET_SP_DPP_ADD(v, 0x122, 0xf);   // row_ror:2
    ONET_SP_DPP_ADD(v, 0x121, 0xf);   // row_ror:1
    ONET_SP_DPP_ADD(v, 0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    return v;
}
#undef ONET_SP_DPP_ADD

struct SpCfg {
    static constexpr int NW = 8, NT = 2, TW = 32, CO_T = 64;
    static constexpr int ROWS = NW * NT;                                // 16 image rows per tile
    static constexpr int IN_ROWS = ROWS + 2, IN_COLS = TW + 2;
    static constexpr int NPIX = IN_ROWS * IN_COLS;                      // 612 halo pixels
    static constexpr int NROUND = (NPIX + 31) / 32;                     // 20 wave-rounds of 32 pixels x 2 halves
    static constexpr int NPIXP = NROUND * 32;                           // 640 pixel slots per half
    static constexpr int W_PART = 9 * 2 * CO_T;                         // 1152 slots per part
    static constexpr int W_SLOTS = 2 * W_PART;                          // hi | mid
    static constexpr int NWI = (W_SLOTS + 511) / 512;                   // 5
    static constexpr int IN_PART = 2 * NPIXP;                           // [half][pixel]
    static constexpr int BUF_SLOTS = W_SLOTS + 2 * IN_PART;             // 4864 slots = 76 KB
    static constexpr int LDS_BYTES = 2 * BUF_SLOTS * 16;                // two chunk buffers: 152 KB
    static constexpr int NB = (NT - 1) + 3;                             // distinct B row-fragments per horizontal tap
};

// ---- shared by conv3x3_split_kernel, conv3x3_split_pre_kernel and conv3x3_pre16_kernel: the persistent tile walk

// tiles of this block: every XCD (blockIdx % 8) owns a contiguous range of the tile list; its blocks stride through the range.
// Tile list order: OUTPUT-CHANNEL tile fastest, then x, y, image -- the Cout / 64 blocks that need the same input tile run on
// one XCD at the same time and share it in that L2 (with the channel tile slowest every one of the Cout / 64 passes over the
// batch streamed the whole input from HBM again: 1.8 x the compulsory bytes per launch on average); the weight slices of
// all channel tiles (<= 9 MB) then live in L2 / MALL instead of one slice at a time
__device__ __forceinline__ void sp_tile_range(int ntiles, int& t_first, int& t_end, int& t_stride) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int q = ntiles >> 3, r = ntiles & 7;
    const int start = xcd * q + min(xcd, r);
    t_stride = (gridDim.x + 7 - xcd) >> 3;
    t_first = start + j;
    t_end = start + q + (xcd < r ? 1 : 0);
}
// entry v of the tile list: output channels co0 .. + 63 of rows y0 .. + 15, pixels x0 .. + 31 of image b (W16: of image PAIR b)
struct SpTile {
    int co0, tx, ty, b, y0, x0;
};
__device__ __forceinline__ SpTile sp_tile(int v, int coTiles, int tilesX, int tilesY) {
    SpTile t;
    t.co0 = (v % coTiles) * SpCfg::CO_T;             // output-channel tile fastest: see the tile order note above
    v /= coTiles;
    t.tx = v % tilesX;
    v /= tilesX;
    t.ty = v % tilesY;
    t.b = v / tilesY;
    t.y0 = t.ty * SpCfg::ROWS;
    t.x0 = t.tx * SpCfg::TW;
    return t;
}

// PERSISTENT blocks: a block walks over output tiles and the chunk pipeline -- global loads two 16-channel
// chunks ahead of the MFMAs, LDS commit one ahead -- runs ACROSS tile boundaries.
// ST: the forward of a Conv-BatchNorm pair (OV:47-48, 51-52) also emits the BatchNorm statistics of its output, one (n, mean,
// M2) record per tile and channel from the final accumulators (pivot-shifted sums per wave, the eight waves merged through LDS).
// NORM (normalise on load): the input is the pre-activation z of the unit below and the staging threads apply that unit's
// BatchNorm + ReLU -- max(fma(z - mean, scale, shift), 0), the expression of bn_relu_apply_kernel, so the operand is bit for
// bit the activation that pass would have written -- before splitting; zero padding stays zero.  The second convolution of a
// DoubleConv (OV:51) then needs no materialised activation of the first (OV:49): one write and one read of the tensor less.
template <bool ST, bool NORM, bool F16>
__global__ __launch_bounds__(512, 2) void conv3x3_split_kernel(SpArgs a) {
    using C = SpCfg;
    constexpr int NT = C::NT, IN_COLS = C::IN_COLS, NWI = C::NWI, CO_T = C::CO_T, NPIXP = C::NPIXP, NB = C::NB;
    constexpr int BUF = C::BUF_SLOTS, W_PART = C::W_PART, IN_PART = C::IN_PART, TW = C::TW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    u32x4s* lds = reinterpret_cast<u32x4s*>(smem_s);                   // [2 buffers][weights hi|mid | input hi|mid]

    int t_first, t_end, t_stride;                                      // tile list order: see sp_tile_range
    sp_tile_range(a.tilesX * a.tilesY * a.B * a.coTiles, t_first, t_end, t_stride);
    if (t_first >= t_end) return;

    const int tid = threadIdx.x, lane = tid & 63, wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const int HW = a.H * a.W;
    const int nchunks = a.Cin >> 4;
    // F16: the operand scales (powers of two): x by its magnitude slots, the weights by the pack's own (stored behind the pack)
    float xs_inv = 1.f;
    const float xs_scale = F16 ? amax_scale(amax_read(a.x_amax), a.x_always != 0, xs_inv) : 1.f;
    const float acc_scale = F16 ? xs_inv * reinterpret_cast<const float*>(a.wq + (int64_t)a.Cin * 2 * 9 * a.Cout)[1] : 1.f;

    const __amdgpu_buffer_rsrc_t wr = s_rsrc(a.wq, (int64_t)a.Cin * 2 * 9 * a.Cout * 2);
    const unsigned in_step = (unsigned)(16 * HW * 4), w_step = (unsigned)(2 * 9 * 2 * a.Cout * 16);
    const unsigned plane = (unsigned)(HW * 4);

    // ---- staging side: runs two chunks ahead of the compute side, across tiles.  Input roles (wave-uniform):
    //   waves 0..4, item it = tid < 288 = (half h, halo row r, 4-pixel group g):  8 x buffer_load_dwordx4 -- the 4 interior pixels
    //              x0 + 4g .. + 3 of row r in the 8 channel planes of half h -- give the 4 slots (8 channels x 1 pixel) of those pixels;
    //   waves 5..6, item tid - 320 < 72 = (half, row, side): the halo column x0 - 1 / x0 + 32, 8 x buffer_load_dword, one slot.
    // (Round 3's first version loaded every slot as 8 dwords, one pixel per lane: 24 VMEM instructions per thread and chunk, 232 per
    // block; a timing build without them ran 19-22 % faster.  Now 8 per staging thread, ~100 per block, the same bytes.)
    // Requires W % 4 == 0 and 16-byte aligned image rows (host-checked): a float4 is entirely inside or outside the image.
    // Weight slots i = tid + 512 k = (part, tap, half, co) -> 16 bytes of the slice [chunk][part][tap][half][co][8].
    unsigned in_off, w_off[NWI];
    const int role = wn < 5 ? 0 : (wn < 7 ? 1 : 2);                    // 0 interior, 1 halo column, 2 none
    const int it = role == 0 ? tid : tid - 320;
    const int it_h = role == 0 ? it / 144 : it / 36;
    const int it_r = role == 0 ? (it % 144) / 8 : (it % 36) / 2;
    const int it_g = role == 0 ? (it & 7) : (it & 1);                  // 4-pixel group / side
    const bool it_ok = role == 0 ? it < 288 : (role == 1 && it < 72);
    __amdgpu_buffer_rsrc_t xr;
    int st_tile = t_first, st_chunk = 0, st_b = 0;
    unsigned cin_bytes = 0, cw_bytes = 0;
    // NORM: the BatchNorm coefficients of a chunk's 16 channels travel beside its data -- 48 floats (mean, scale, shift) fetched
    // by the one wave without a staging role and parked in LDS [chunk buffer][half][channel][4], where the staging threads pick
    // them up at commit time (per-lane vector loads would double the staging VMEM count, 48 scalar loads spilled the SGPR file)
    float* const coef = reinterpret_cast<float*>(lds + 2 * BUF) + (ST ? C::NW * 64 * 2 : 0);
    float pend_cv = 0.f;
    bool pend_keep = false;                          // validity of the item whose loads are in flight
    auto setup_stage = [&]() __attribute__((always_inline)) {
        const bool live = st_tile < t_end;
        const auto [co0, tx, ty, b, y0, x0] = sp_tile(live ? st_tile : t_first, a.coTiles, a.tilesX, a.tilesY);
        st_b = b;
        xr = s_rsrc(a.x + (int64_t)b * a.x_bs, (int64_t)a.Cin * HW * 4);
        {
            const int yy = y0 - 1 + it_r;
            const int xx = role == 0 ? x0 + 4 * it_g : (it_g ? x0 + TW : x0 - 1);
            const bool ok = live && it_ok && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            in_off = ok ? (unsigned)(((it_h * 8) * HW + yy * a.W + xx) * 4) : OOB_S;
        }
#pragma unroll
        for (int k = 0; k < NWI; ++k) {
            const int i = tid + 512 * k;
            const int co = i & (CO_T - 1), pth = i >> 6;               // pth = (part * 9 + tap) * 2 + half
            const bool ok = live && (i < C::W_SLOTS) && (co0 + co < a.Cout);
            w_off[k] = ok ? (unsigned)((pth * a.Cout + co0 + co) * 16) : OOB_S;
        }
    };
    auto advance = [&]() __attribute__((always_inline)) {
        ++st_chunk;
        cin_bytes += in_step;
        cw_bytes += w_step;
        if (st_chunk == nchunks) {
            st_chunk = 0;
            cin_bytes = cw_bytes = 0;
            st_tile += t_stride;
            setup_stage();                           // past the last tile: every slot out of range -> zeros, no traffic
        }
    };

    u32x4s xin[8];                                   // plane c of the item: 4 pixels (interior) or 1 pixel in lane 0 (halo column)
    u32x4s wv[NWI];
    // loads of planes [c0, c1) of this thread's item; the chunk / plane part of the address is wave-uniform and rides in the
    // instruction's scalar offset, the per-lane part alone decides the range check (OOB_S -> 0)
    auto issue_in = [&](int c0, int c1) __attribute__((always_inline)) {
        if (NORM && c0 == 0) {
            pend_keep = in_off != OOB_S;
            if (wn == 7 && lane < 48) {              // lane = kind * 16 + channel; rows of `save`: 0 mean, 2 scale, 3 shift
                const int k = lane >> 4, row = k == 0 ? 0 : k + 1;
                pend_cv = st_tile < t_end ? a.nsave[(int64_t)((st_b / a.nimg) * 4 + row) * a.Cin + st_chunk * 16 + (lane & 15)] : 0.f;
            }
        }
        if (role == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c >= c0 && c < c1) xin[c] = __builtin_amdgcn_raw_buffer_load_b128(xr, in_off, (int)(cin_bytes + c * plane), 0);
        } else if (role == 1) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c >= c0 && c < c1) xin[c][0] = __builtin_amdgcn_raw_buffer_load_b32(xr, in_off, (int)(cin_bytes + c * plane), 0);
        }
    };
    auto issue_w = [&](int k0, int k1) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < NWI; ++k)
            if (k >= k0 && k < k1) wv[k] = __builtin_amdgcn_raw_buffer_load_b128(wr, w_off[k], (int)cw_bytes, 0);
    };
    u32x4s* const w_st = lds + tid;                                     // + 512 k          (+ buffer * BUF)
    // slot of halo pixel (row r, column c) = W_SLOTS + part * IN_PART + half * NPIXP + r * IN_COLS + c
    u32x4s* const in_st = lds + C::W_SLOTS + it_h * NPIXP + it_r * IN_COLS + (role == 0 ? 1 + 4 * it_g : (it_g ? IN_COLS - 1 : 0));
    // pixels [p0, p1) of the item (interior: 4 pixels, halo column: pixel 0 only): 8 channels -> one slot per part
    auto commit_in = [&](int buf, int p0, int p1) __attribute__((always_inline)) {
        if (role == 2 || !it_ok) return;
        f32x4s f[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = __builtin_bit_cast(f32x4s, xin[c]);      // (re-typed as a whole: see commit_dz below)
        if constexpr (NORM) {
            // channel pairs outermost (a dword of a slot = two neighbouring channels): six coefficients live at a time
            const f32x4s* cfp = reinterpret_cast<const f32x4s*>(coef) + (buf * 2 + it_h) * 8;
            u32x4s hi[4], mid[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4s ca = cfp[2 * c], cb = cfp[2 * c + 1];
#pragma unroll
                for (int px = 0; px < 4; ++px) {
                    if (px < p0 || px >= p1 || (role == 1 && px > 0)) continue;
                    float va = fmaxf(fmaf(f[2 * c][px] - ca[0], ca[1], ca[2]), 0.f);
                    float vb = fmaxf(fmaf(f[2 * c + 1][px] - cb[0], cb[1], cb[2]), 0.f);
                    va = pend_keep ? va : 0.f;               // outside the image: the convolution's zero padding
                    vb = pend_keep ? vb : 0.f;
                    unsigned h, m;
                    if constexpr (F16) split2h_s(va, vb, xs_scale, h, m);
                    else split2(va, vb, h, m);
                    hi[px][c] = h;
                    mid[px][c] = m;
                }
            }
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                if (px < p0 || px >= p1 || (role == 1 && px > 0)) continue;
                in_st[buf * BUF + px] = hi[px];
                in_st[buf * BUF + px + IN_PART] = mid[px];
            }
            return;
        }
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            if (px < p0 || px >= p1 || (role == 1 && px > 0)) continue;
            u32x4s hi, mid;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                unsigned h, m;
                if constexpr (F16) split2h_s(f[2 * c][px], f[2 * c + 1][px], xs_scale, h, m);
                else split2(f[2 * c][px], f[2 * c + 1][px], h, m);
                hi[c] = h;
                mid[c] = m;
            }
            in_st[buf * BUF + px] = hi;
            in_st[buf * BUF + px + IN_PART] = mid;
        }
    };
    auto commit_w = [&](int buf, int k0, int k1) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < NWI; ++k)
            if (k >= k0 && k < k1 && tid + 512 * k < C::W_SLOTS) w_st[buf * BUF + 512 * k] = wv[k];
    };

    auto commit_coef = [&](int cb) __attribute__((always_inline)) {
        if (NORM && wn == 7 && lane < 48) coef[((cb * 2 + ((lane >> 3) & 1)) * 8 + (lane & 7)) * 4 + (lane >> 4)] = pend_cv;
    };

    // fragments: A (weights) slot = part * W_PART + (tap * 2 + kh) * 64 + m * 32 + l31;
    //            B (input)   slot = W_SLOTS + part * IN_PART + kh * NPIXP + (2 wn + j) * IN_COLS + l31 + kx
    const u32x4s* const a_ptr = lds + kh * CO_T + l31;
    const u32x4s* const b_ptr = lds + C::W_SLOTS + kh * NPIXP + (wn * NT) * IN_COLS + l31;

    setup_stage();
    issue_in(0, 8);
    issue_w(0, NWI);
    if constexpr (NORM) {
        commit_coef(0);
        __syncthreads();
    }
    commit_in(0, 0, 4);
    commit_w(0, 0, NWI);
    advance();
    issue_in(0, 8);                                  // second chunk (or the first of the next tile)
    issue_w(0, NWI);
    commit_coef(1);
    __syncthreads();
    int buf = 0;
    for (int tile = t_first; tile < t_end; tile += t_stride) {
        f32x16 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

        for (int c = 0; c < nchunks; ++c) {
            const u32x4s* const ab = a_ptr + buf * BUF;
            const u32x4s* const bb = b_ptr + buf * BUF;
            // Fragment reads run ONE tap ahead of the MFMAs that consume them (two register sets), the taps in kx-major order
            // so that the NB row-fragments of a horizontal shift serve its three vertical taps; the row-fragments of the next
            // shift are fetched during the three taps of the current one.  [part]: 0 = hi, 1 = mid.
            u32x4s Aq[2][2][2], Bq[2][NB][2];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                Bq[0][j][0] = bb[j * IN_COLS];
                Bq[0][j][1] = bb[j * IN_COLS + IN_PART];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                Aq[0][m][0] = ab[m * 32];
                Aq[0][m][1] = ab[m * 32 + W_PART];
            }
#pragma unroll
            for (int idx = 0; idx < 9; ++idx) {
                const int kx = idx / 3, ky = idx % 3;
                if (idx < 8) {
                    const int nt = ((idx + 1) % 3) * 3 + (idx + 1) / 3;
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        Aq[(idx + 1) & 1][m][0] = ab[nt * 2 * CO_T + m * 32];
                        Aq[(idx + 1) & 1][m][1] = ab[nt * 2 * CO_T + m * 32 + W_PART];
                    }
                }
                if (kx < 2) {
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        if (j % 3 == ky) {
                            Bq[(kx + 1) & 1][j][0] = bb[j * IN_COLS + kx + 1];
                            Bq[(kx + 1) & 1][j][1] = bb[j * IN_COLS + kx + 1 + IN_PART];
                        }
                }
                // Staging, spread over the taps so that no wave sits in a burst of VMEM issues while its SIMD partner does the same:
                // the other buffer was last read one chunk ago (barrier since), so the chunk after this one goes in piece by piece
                // -- and once an item's pixels are committed its registers take the loads of the chunk after that (every load
                // keeps most of a chunk of MFMAs between issue and use).  Inputs: pixels 0, 1 at tap 0, pixels 2, 3 at tap 1, the
                // eight plane loads two per tap at taps 2..5; weights: commit + reload of slot k at taps 4..8.
                if (idx == 0) advance();
                if (idx == 0) commit_in(buf ^ 1, 0, 2);
                if (idx == 1) commit_in(buf ^ 1, 2, 4);
                if (idx >= 2 && idx <= 5) issue_in(2 * (idx - 2), 2 * (idx - 2) + 2);
                if (idx >= 4) {
                    commit_w(buf ^ 1, idx - 4, idx - 3);
                    issue_w(idx - 4, idx - 3);
                }
                if (idx == 8) commit_coef(buf);      // for the chunk whose loads went out at taps 2..5: committed into `buf` next
                __builtin_amdgcn_sched_barrier(0);
                const int tap = ky * 3 + kx;
                (void)tap;
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        // smallest terms first: the two cross terms, then hi * hi
                        if constexpr (F16) {
                            const f16x8 ah = __builtin_bit_cast(f16x8, Aq[idx & 1][m][0]), am = __builtin_bit_cast(f16x8, Aq[idx & 1][m][1]);
                            const f16x8 bh = __builtin_bit_cast(f16x8, Bq[kx & 1][n + ky][0]), bm = __builtin_bit_cast(f16x8, Bq[kx & 1][n + ky][1]);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(am, bh, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bm, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[m][n], 0, 0, 0);
                        } else {
                            const bf16x8 ah = __builtin_bit_cast(bf16x8, Aq[idx & 1][m][0]), am = __builtin_bit_cast(bf16x8, Aq[idx & 1][m][1]);
                            const bf16x8 bh = __builtin_bit_cast(bf16x8, Bq[kx & 1][n + ky][0]), bm = __builtin_bit_cast(bf16x8, Bq[kx & 1][n + ky][1]);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[m][n], 0, 0, 0);
                        }
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            buf ^= 1;
        }

        if constexpr (F16) {                         // undo the operands' power-of-two scales (exact)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][n][r] *= acc_scale;
        }
        const auto [co0, tx, ty, b, y0, x0] = sp_tile(tile, a.coTiles, a.tilesX, a.tilesY);
        if constexpr (ST) {
            float* sc = reinterpret_cast<float*>(lds + 2 * BUF);       // [8 waves][64 channels][mean, M2]
            constexpr float npw = (float)(NT * 32), inv_npw = 1.f / npw;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // lanes 0-31 hold 32 pixels of channel c, lanes 32-63 of channel c + 4; pivot = the wave's first pixel
                    const int piv = __builtin_bit_cast(int, acc[m][0][r]);
                    const float p0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(piv, 0));
                    const float p1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(piv, 32));
                    const float pv = kh ? p1 : p0;
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const float d = acc[m][n][r] - pv;
                        s1 += d;
                        s2 = fmaf(d, d, s2);
                    }
                    s1 = sp_half_sum(s1);
                    s2 = sp_half_sum(s2);
                    if (l31 == 31) {
                        const int cl = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                        sc[(wn * 64 + cl) * 2] = fmaf(s1, inv_npw, pv);
                        sc[(wn * 64 + cl) * 2 + 1] = fmaxf(fmaf(-s1 * inv_npw, s1, s2), 0.f);
                    }
                }
            __syncthreads();
            if (tid < 64 && co0 + tid < a.Cout) {
                float mw[8], qw[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    mw[w] = sc[(w * 64 + tid) * 2];
                    qw[w] = sc[(w * 64 + tid) * 2 + 1];
                }
                const float mean = 0.125f * (((mw[0] + mw[1]) + (mw[2] + mw[3])) + ((mw[4] + mw[5]) + (mw[6] + mw[7])));
                float m2 = ((qw[0] + qw[1]) + (qw[2] + qw[3])) + ((qw[4] + qw[5]) + (qw[6] + qw[7]));
#pragma unroll
                for (int w = 0; w < 8; ++w) m2 = fmaf(npw * (mw[w] - mean), mw[w] - mean, m2);
                const int64_t nblk = (int64_t)a.B * a.tilesY * a.tilesX;
                const int64_t blk = ((int64_t)b * a.tilesY + ty) * a.tilesX + tx;
                float* sp = a.stats + ((int64_t)(co0 + tid) * nblk + blk) * 3;
                sp[0] = 8.f * npw;
                sp[1] = mean;
                sp[2] = m2;
            }
            __syncthreads();                         // the scratch is rewritten by the next tile
        }
        float* zb = a.z + (int64_t)b * a.z_bs;
        const int xo = x0 + l31;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int yo = y0 + wn * NT + n;
                if (yo < a.H && xo < a.W) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                        if (co < a.Cout) zb[(int64_t)co * HW + (int64_t)yo * a.W + xo] = acc[m][n][r];
                    }
                }
            }
    }
}


// ------------------------------------------------------------------ pre-split operands (round 4)
// The activation arrives ALREADY split, in the slot layout the tile wants:
//     xs [B][C/8][H][part 2][W][8] 16-bit   (part 0 = hi, 1 = mid; fp16 or bf16; 4 bytes per element -- the fp32 tensor's footprint)
// written by the producers (bn.hip: BatchNorm + ReLU apply / pooling, BatchNorm backward apply; convt_gemm.hip epilogue).  The
// MFMA kernel's staging is then a COPY: every 16-byte slot of the halo tile and of the weight slice goes HBM -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds: no staging registers, no conversion VALU, no ds_write -- the round-3 kernel spent 19-26 % of its
// time there, with 4-way bank conflicts on its ds_write_b128), one chunk ahead of the MFMAs into the other chunk buffer.
typedef int i32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4s sp_rsrc4(const void* base, int64_t bytes) {
    const uint64_t p = reinterpret_cast<uint64_t>(base);
    i32x4s r;
    r.x = (int)(p & 0xffffffffu);
    r.y = (int)((p >> 32) & 0xffffu);
    r.z = bytes > 0x7fffffffll ? 0x7fffffff : (int)bytes;
    r.w = 0x00020000;
    return r;
}
// LDS-DMA of 64 x 16 bytes: lane l's 16 bytes at (rsrc base + voff + soff) land at LDS byte address lds_base + 16 l; a lane
// whose address is out of range (voff = OOB_S) writes zeros.  Inline asm: the compiler must not see a load (it would order every
// later ds_read behind a vmcnt(0)); m0 is restored because the compiler does not know it was touched.
__device__ __forceinline__ void sp_dma16(i32x4s rsrc, unsigned lds_base, unsigned voff, unsigned soff) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(lds_base), "s"(soff)
                 : "memory");
}

// fp32 NCHW -> the slot layout above (tests, tools, and producers that have no fused variant yet)
// f16 == 2: plain bf16, one part: xs [B][C/8][H][W][8]
// slots != NULL: the tensor's magnitude slots -- the guard scale of amax_scale(.., always = false) multiplies `scale` (what a fused
// producer with the same slots would have applied; the consumer undoes it from the same slots)
__global__ void split_pack_act_kernel(const float* __restrict__ x, int64_t x_bs, unsigned* __restrict__ xs, int64_t xs_bs, int B, int C8,
                                      int H, int W, int f16, float scale, const unsigned* __restrict__ slots) {
    if (slots) {
        float inv;
        scale *= amax_scale(amax_read(slots), false, inv);
    }
    const int64_t n = (int64_t)B * C8 * H * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % W);
        int64_t r = i / W;
        const int y = (int)(r % H);
        r /= H;
        const int c8 = (int)(r % C8), b = (int)(r / C8);
        const float* src = x + (int64_t)b * x_bs + ((int64_t)c8 * 8 * H + y) * W + xx;
        u32x4s hi, mid;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float va = src[(int64_t)(2 * c) * H * W] * scale, vb = src[(int64_t)(2 * c + 1) * H * W] * scale;
            unsigned h, m;
            if (f16 == 1) split2h(va, vb, h, m);
            else split2(va, vb, h, m);
            hi[c] = h;
            mid[c] = m;
        }
        if (f16 == 2) {
            reinterpret_cast<u32x4s*>(xs + (int64_t)b * xs_bs)[((int64_t)c8 * H + y) * W + xx] = hi;
            continue;
        }
        u32x4s* dst = reinterpret_cast<u32x4s*>(xs + (int64_t)b * xs_bs) + (((int64_t)c8 * H + y) * 2) * W + xx;
        dst[0] = hi;
        dst[W] = mid;
    }
}

struct SpPreArgs {
    const void* xs;       // pre-split activation, slot layout
    int64_t xs_bs;        // batch stride in 4-byte units (= C * H * W for a dense tensor)
    const __bf16* wq;     // [Cin/16][2][9][2][Cout][8]
    float* z;
    int64_t z_bs;
    int B, Cin, Cout, H, W, tilesX, tilesY, coTiles;
    float* stats;         // ST: BatchNorm partials (as conv3x3_split_kernel)
    const unsigned* x_slots;   // magnitude slots the producer scaled xs by (NULL: unscaled); x_always: the rule it used (amax_scale)
    int x_always;
    const unsigned* x_slots2;  // a concat buffer has two producers: channels >= split_ch were scaled by these slots (NULL: unscaled)
    int split_ch;              // 0: one group
    // RD (conv3x3_pre16_kernel, input-gradient launches): the output z IS the gradient da of the Conv-BatchNorm-ReLU unit below; its
    // BatchNorm-backward reduce pass rides in the epilogue: rd_z = that unit's pre-activation [B][Cout][H][W] fp32, rd_save its
    // coefficients [G][4][Cout] (groups of rd_gimg images; 0: one group), rd_rec [tiles][Cout][4] receives (sum dy, 0, sum dy xhat, 0)
    // per tile (bn_relu_bwd_reduce_kernel's record format), rd_amax (may be NULL) the magnitude slots of da.
    const float* rd_z = nullptr;
    union { int64_t rd_z_bs = 0; int64_t pl_y_bs; };
    const float* rd_save = nullptr;
    union { int rd_gimg = 0; int n_img; };     // (n_img: the image count of an activation launch on image-pair tiles, see below)
    float* rd_rec = nullptr;
    unsigned* rd_amax = nullptr;
    // conv3x3_pre16_kernel, plain bf16 operands (BASELINE configs[2]): z16 -- the output z is STORED as bf16 (rounded once, to nearest
    // even; the statistics epilogue still reads the fp32 accumulators), z_bs in elements; rd_z16 -- rd_z is such a bf16 tensor
    int z16 = 0, rd_z16 = 0;
    // conv3x3_split_pre_kernel, fp16 (hi | mid) parts (round 5): output channels >= zP_ch0 (a multiple of 64) are NOT written to z but,
    // pre-split, to zP [B][(Cout - zP_ch0) / 8][H][2][W][8] (batch stride zP_bs in 4-byte units) as parts of 2^k z, k by the `always`
    // rule from the bound in zP_slots: the input gradient of a decoder block's first convolution hands the up-sampled half of the
    // concat gradient to the ConvTranspose2d backward GEMMs in their operand form
    void* zP = nullptr;
    int64_t zP_bs = 0;
    int zP_ch0 = 0;
    const unsigned* zP_slots = nullptr;
    // conv3x3_split_pre_kernel<false, 1, false, ACT = true> (eval-mode inference): the epilogue applies a fixed BatchNorm + ReLU to the
    // accumulator tile -- a = max(0, fma(z - mean, sc, sh)) with act_save [4][Cout] in bn_eval_coeffs' format, bn_relu_apply_split's
    // arithmetic -- and EVERY channel leaves as slots through zP (zP_ch0 = 0), as parts of 2^k a with k by the GUARD rule (always = false)
    // from the bound in zP_slots.  z is never written.  act_amax (may be NULL): magnitude slots that receive the exact max a;
    // act_a (may be NULL): the activation in fp32 NCHW too, batch stride act_a_bs
    const float* act_save = nullptr;
    unsigned* act_amax = nullptr;
    float* act_a = nullptr;
    int64_t act_a_bs = 0;
    // conv3x3_pre16_kernel<false, PM, false, false, false, HEAD = true> (labels-only inference, Cout == 64: one channel tile holds every
    // output channel of a pixel): the epilogue forms h = max(0, fma(z - mean, sc, sh)) with act_save as above and reduces it against
    // hd_L [B][Cout][H][W] fp32 (batch stride hd_L_bs) over the channels: hd_V [B][H][W] = sum_c L[c] h[c] is ALL the launch writes
    union { const float* hd_L = nullptr; void* pl_P; };
    union { int64_t hd_L_bs = 0; int64_t pl_P_bs; };
    union { float* hd_V = nullptr; float* pl_y; };
    // POOL (on top of ACT: an encoder block's second unit, the one in front of a max-pool): besides every store of ACT the epilogue forms
    // m = the maximum of each 2 x 2 window of a (fmaxf; a tile starts on even rows and columns and a wave owns two adjacent rows, so no
    // window leaves a wave) and writes it as slots -- pl_P [B][Cout/8][H/2][parts][W/2][8], the parts of 2^k m with zP's k, batch stride
    // pl_P_bs in 4-byte units -- and / or as fp32 NCHW -- pl_y [B][Cout][H/2][W/2], batch stride pl_y_bs: what
    // bn_relu_apply_pool_split_kernel writes from a stored z, bit for bit.  The four fields share the storage of hd_L, hd_L_bs, hd_V and
    // rd_z_bs above -- epilogues POOL excludes (HEAD, RD) -- so that the kernel-argument block, and with it the code of every other
    // instance, keeps its size and layout
    // conv3x3_pre16_kernel<false, 2, W16 = true, false, ACT = true> (round 16, include/onet_hip_pairs.h: the eval plan's bottom level, maps
    // of any H and 0 < W <= 16): the activation epilogue on image-pair tiles.  B counts the cdiv(n_img, 2) pairs and n_img (the storage
    // of rd_gimg: RD and ACT exclude each other) the images -- with an odd count the last tile holds ONE image: its second half stages
    // the out-of-range offset, stores nothing, and the tile's buffer resource ends with the first image
    // conv3x3_split_pre_kernel<false, 1, W16 = true, ACT = true, false, RAG = true> (round 18, include/onet_hip_split_pairs.h): the same
    // on fp16 (hi | mid) parts -- B and n_img as above, zP_slots / act_amax as on the ragged instance (the record masks absent images too)
};

// PM: 0 = bf16 (hi | mid) parts, 1 = fp16 (hi | mid) parts -- three MFMAs per term on 16-channel chunks; 2 = PLAIN bf16 operands
// (BASELINE configs[2]'s bf16 MFMA conv path: xs [B][C/8][H][W][8] bf16, one part): the same LDS image and DMA schedule with the
// "part" index standing for the second 16 channels of a 32-channel chunk, two MFMAs per term (one per 16 channels).
// W16: maps 16 pixels wide (the U-Net's 16-pixel level): a tile's 32 pixel columns are TWO IMAGES side by side, each with its own halo
// columns in the LDS image (18 + 18 columns), so a horizontal tap never reads the neighbour image; a.B counts image PAIRS.
template <bool W16> struct SpPreCfg {
    static constexpr int NW = 8, NT = 16 / NW, TW = 32, CO_T = 64, ROWS = NW * NT;     // NW waves per block: two rows per wave
    static constexpr int IN_ROWS = ROWS + 2, IN_COLS = W16 ? 36 : 34;
    static constexpr int NPIX = IN_ROWS * IN_COLS;                      // 612 / 648 halo pixels
    static constexpr int NPIXP = W16 ? 656 : 640;                       // pixel slots per half (4 NPIXP = whole 64-slot DMA pieces)
    static constexpr int W_PART = 9 * 2 * CO_T, W_SLOTS = 2 * W_PART, NWI = (W_SLOTS + NW * 64 - 1) / (NW * 64);
    static constexpr int IN_PART = 2 * NPIXP;
    static constexpr int BUF_SLOTS = W_SLOTS + 2 * IN_PART;             // 76 / 77 KB
    static constexpr int LDS_BYTES = 2 * BUF_SLOTS * 16;
    static constexpr int NB = (NT - 1) + 3;
    static constexpr int LAST_TAP = 4;                                  // the next chunk's DMA pieces go out during taps 0 .. LAST_TAP
    static_assert(CO_T == SpCfg::CO_T && ROWS == SpCfg::ROWS && TW == SpCfg::TW, "sp_tile: one tile shape for every kernel of the family");
};
template <int CTRL> __device__ __forceinline__ float dpp_max(float x) {     // max(x, x of the lane DPP control CTRL selects)
    return fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false)));
}
// RAG (round 14, the fp16 ragged entries of include/onet_hip_ragged_split.h): the activation epilogue on maps that are not made of full
// tiles.  The staging (the out-of-range offset), the tile counts (cdiv) and every store (yo < H && xo < W; the pooled ones: pst) already
// are ragged-ready, and both lane exchanges (v_permlane32_swap, the pooling's DPP step) run outside those guards, in every lane.  What
// needs code is the exact-maximum record (act_amax): an out-of-map accumulator is relu(bn(.)) of a partial or empty sum -- not zero --
// and must not enter the maximum the next layer's bound starts from.
template <bool ST, int PM, bool W16, bool ACT = false, bool POOL = false, bool RAG = false>
__global__ __launch_bounds__(SpPreCfg<W16>::NW * 64, SpPreCfg<W16>::NW / 4) void conv3x3_split_pre_kernel(SpPreArgs a) {
    constexpr bool F16 = PM == 1;
    static_assert(!RAG || ACT, "conv3x3_split_pre_kernel: the ragged instance is the activation epilogue's (masked exact maximum)");
    static_assert(!ACT || (PM == 1 && !ST && (!W16 || (RAG && !POOL))),
                  "conv3x3_split_pre_kernel: the activation epilogue goes with the fp16 slot store; on image-pair tiles: the masked record, no pooled twin");
    static_assert(!POOL || ACT, "conv3x3_split_pre_kernel: the pooled stores ride on the activation epilogue");
    using C = SpPreCfg<W16>;
    constexpr bool PAIRS = W16 && ACT;                                 // the activation epilogue on image-pair tiles (SpPreArgs::n_img)
    constexpr int NT = C::NT, IN_COLS = C::IN_COLS, NWI = C::NWI, CO_T = C::CO_T, NPIXP = C::NPIXP, NB = C::NB;
    constexpr int BUF = C::BUF_SLOTS, W_PART = C::W_PART, IN_PART = C::IN_PART;
    constexpr int NWV = C::NW, NTH = NWV * 64;
    constexpr int NII = (2 * IN_PART + NTH - 1) / NTH;                     // 5 (6) input DMA rounds per wave and chunk (2560 / 2624 slot positions)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    u32x4s* lds = reinterpret_cast<u32x4s*>(smem_s);                   // [2 buffers][weights hi|mid | input hi|mid]

    int t_first, t_end, t_stride;                                      // tile list order: see sp_tile_range
    sp_tile_range(a.tilesX * a.tilesY * a.B * a.coTiles, t_first, t_end, t_stride);
    if (t_first >= t_end) return;

    const int tid = threadIdx.x, lane = tid & 63, wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const int HW = a.H * a.W;
    const int nchunks = PM == 2 ? a.Cin >> 5 : a.Cin >> 4;

    const i32x4s wr = sp_rsrc4(a.wq, (int64_t)a.Cin * (PM == 2 ? 1 : 2) * 9 * a.Cout * 2);
    float xs_inv = 1.f, xs_inv2 = 1.f;
    (void)amax_scale(amax_read(a.x_slots), a.x_always != 0, xs_inv);
    (void)amax_scale(amax_read(a.x_slots2), a.x_always != 0, xs_inv2);
    // two groups: sum = inv1 A1 + inv2 A2 = inv2 ((inv1 / inv2) A1 + A2): the accumulators are rescaled once, at the first chunk of
    // group 2, by a power of two (1 in every ordinary network: nothing is done then)
    const int split_chunk = a.split_ch ? (PM == 2 ? a.split_ch >> 5 : a.split_ch >> 4) : 0;
    const float grp_ratio = split_chunk ? xs_inv / xs_inv2 : 1.f;
    const float acc_scale = (split_chunk ? xs_inv2 : xs_inv) * (F16 ? reinterpret_cast<const float*>(a.wq + (int64_t)a.Cin * 2 * 9 * a.Cout)[1] : 1.f);
    const unsigned in_step = (unsigned)(16 * HW * 4), w_step = (unsigned)(2 * 9 * 2 * a.Cout * 16);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_s;

    // ---- staging: slot position i = (wn + 8 k) * 64 + lane of the chunk image.  Input k < NII: i = (part * 2 + half) * NPIXP + pix,
    // pix = r * IN_COLS + c (pix >= 612: padding of the image, zeros).  Weights k < NWI: i = (part * 9 + tap) * 2 + half) * 64 + co.
    unsigned in_off[NII], w_off[NWI];
    i32x4s xr;
    int st_tile = t_first, st_chunk = 0;
    unsigned cin_bytes = 0, cw_bytes = 0;
    auto setup_stage = [&]() __attribute__((always_inline)) {
        const bool live = st_tile < t_end;
        const auto [co0, tx, ty, b, y0, x0] = sp_tile(live ? st_tile : t_first, a.coTiles, a.tilesX, a.tilesY);
        // (W16: b is the image PAIR; the resource spans both images, the second one's offset rides in the lane's byte offset)
        // (PAIRS: the last tile of an odd image count holds one image -- the resource ends with it, its second half is out of range)
        const bool img1 = !PAIRS || 2 * b + 1 < a.n_img;
        xr = sp_rsrc4(reinterpret_cast<const unsigned*>(a.xs) + (int64_t)(W16 ? 2 * b : b) * a.xs_bs,
                      (W16 && img1 ? a.xs_bs * 4 : 0) + (int64_t)a.Cin * HW * (PM == 2 ? 2 : 4));
#pragma unroll
        for (int k = 0; k < NII; ++k) {
            const int i = (wn + NWV * k) * 64 + lane;
            const int ph = i / NPIXP, pix = i % NPIXP;                 // ph = part * 2 + half (PM 2: the chunk's channel group 0 .. 3)
            const int r = pix / IN_COLS, c = pix % IN_COLS;
            const int img = W16 ? c / 18 : 0;
            const int yy = y0 - 1 + r, xx = W16 ? c % 18 - 1 : x0 - 1 + c;
            const bool ok = live && i < 2 * IN_PART && pix < C::NPIX && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W && (!PAIRS || img == 0 || img1);
            const unsigned io = W16 ? (unsigned)(img * a.xs_bs * 4) : 0u;
            in_off[k] = !ok ? OOB_S : PM == 2 ? io + (unsigned)(((ph * a.H + yy) * a.W + xx) * 16)
                                              : io + (unsigned)(((((ph & 1) * a.H + yy) * 2 + (ph >> 1)) * a.W + xx) * 16);
        }
#pragma unroll
        for (int k = 0; k < NWI; ++k) {
            const int i = tid + NTH * k;
            const int co = i & (CO_T - 1), pth = i >> 6;
            const bool ok = live && (i < C::W_SLOTS) && (co0 + co < a.Cout);
            w_off[k] = ok ? (unsigned)((pth * a.Cout + co0 + co) * 16) : OOB_S;
        }
    };
    auto advance = [&]() __attribute__((always_inline)) {
        ++st_chunk;
        cin_bytes += in_step;
        cw_bytes += w_step;
        if (st_chunk == nchunks) {
            st_chunk = 0;
            cin_bytes = cw_bytes = 0;
            st_tile += t_stride;
            setup_stage();
        }
    };
    // piece k of the chunk the staging state points at, into chunk buffer `buf`
    auto dma_in = [&](int buf, int k) __attribute__((always_inline)) {
        if ((wn + NWV * k) * 64 < 2 * IN_PART)
            sp_dma16(xr, lds0 + (unsigned)((buf * BUF + C::W_SLOTS + (wn + NWV * k) * 64) * 16), in_off[k], cin_bytes);
    };
    auto dma_w = [&](int buf, int k) __attribute__((always_inline)) {
        if (k < NWI - 1 || wn < (C::W_SLOTS - NTH * (NWI - 1)) / 64)
            sp_dma16(wr, lds0 + (unsigned)((buf * BUF + (wn + NWV * k) * 64) * 16), w_off[k], cw_bytes);
    };

    const u32x4s* const a_ptr = lds + kh * CO_T + l31;
    const u32x4s* const b_ptr = lds + C::W_SLOTS + kh * NPIXP + (wn * NT) * IN_COLS + (W16 ? (l31 >> 4) * 18 + (l31 & 15) : l31);

    setup_stage();
#pragma unroll
    for (int k = 0; k < NII; ++k) dma_in(0, k);
#pragma unroll
    for (int k = 0; k < NWI; ++k) dma_w(0, k);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    float zP_scale = 1.f;
    if constexpr (PM == 1 && !ST && (!W16 || ACT)) {
        float zinv;
        if (a.zP) zP_scale = amax_scale(amax_read(a.zP_slots), !ACT, zinv);
    }
    // ACT: the tile's 64 x (mean, sc, sh) wait in LDS behind the chunk buffers, [tile parity][3][64] floats -- no registers per lane.
    // Threads 0 .. 191 fetch the NEXT tile's while this tile's chunks run (the load lands under the chunk loop's own waits) and commit
    // them at the top of that tile; its chunk barriers publish them.  Two copies: a wave still in the previous tile's epilogue reads
    // the other one (nobody gets two tiles ahead of a barrier)
    [[maybe_unused]] float* const act_cf = reinterpret_cast<float*>(lds + 2 * BUF);
    [[maybe_unused]] float cf_next = 0.f;
    [[maybe_unused]] int cf_par = 0;
    auto act_fetch = [&](int t) __attribute__((always_inline)) {
        if (tid < 192 && t < t_end) {
            const int k = tid >> 6;                                 // 0: mean, 1: sc, 2: sh   (save rows 0, 2, 3)
            cf_next = a.act_save[(int64_t)(k + (k > 0)) * a.Cout + sp_tile(t, a.coTiles, a.tilesX, a.tilesY).co0 + (tid & 63)];
        }
    };
    if constexpr (ACT) act_fetch(t_first);
    for (int tile = t_first; tile < t_end; tile += t_stride) {
        if constexpr (ACT) {
            cf_par ^= 1;
            if (tid < 192) act_cf[cf_par * 192 + tid] = cf_next;
            act_fetch(tile + t_stride);
        }
        f32x16 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

        for (int c = 0; c < nchunks; ++c) {
            if (split_chunk && c == split_chunk && grp_ratio != 1.f) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[m][n][r] *= grp_ratio;
            }
            const u32x4s* const ab = a_ptr + buf * BUF;
            const u32x4s* const bb = b_ptr + buf * BUF;
            u32x4s Aq[2][2][2], Bq[2][NB][2];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                Bq[0][j][0] = bb[j * IN_COLS];
                Bq[0][j][1] = bb[j * IN_COLS + IN_PART];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                Aq[0][m][0] = ab[m * 32];
                Aq[0][m][1] = ab[m * 32 + W_PART];
            }
#pragma unroll
            for (int idx = 0; idx < 9; ++idx) {
                const int kx = idx / 3, ky = idx % 3;
                if (idx < 8) {
                    const int nt = ((idx + 1) % 3) * 3 + (idx + 1) / 3;
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        Aq[(idx + 1) & 1][m][0] = ab[nt * 2 * CO_T + m * 32];
                        Aq[(idx + 1) & 1][m][1] = ab[nt * 2 * CO_T + m * 32 + W_PART];
                    }
                }
                if (kx < 2) {
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        if (j % 3 == ky) {
                            Bq[(kx + 1) & 1][j][0] = bb[j * IN_COLS + kx + 1];
                            Bq[(kx + 1) & 1][j][1] = bb[j * IN_COLS + kx + 1 + IN_PART];
                        }
                }
                // the other chunk buffer was last read one chunk ago (barrier since): the next chunk's slots go in by DMA, a piece
                // or two per tap during the first taps, so that they have the rest of the chunk's MFMAs to land
                if (idx == 0) advance();
                {
                    constexpr int NPIECE = NII + NWI, PER = (NPIECE + C::LAST_TAP) / (C::LAST_TAP + 1);
#pragma unroll
                    for (int q = 0; q < PER; ++q) {
                        const int pc = idx * PER + q;
                        if (idx <= C::LAST_TAP && pc < NPIECE) {
                            if (pc & 1) { if (pc / 2 < NWI) dma_w(buf ^ 1, pc / 2); else dma_in(buf ^ 1, pc - NWI); }
                            else { if (pc / 2 < NII) dma_in(buf ^ 1, pc / 2); else dma_w(buf ^ 1, pc - NII); }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        if constexpr (PM == 2) {         // plain bf16: channels 0-15 of the chunk, then 16-31
                            const bf16x8 a0 = __builtin_bit_cast(bf16x8, Aq[idx & 1][m][0]), a1 = __builtin_bit_cast(bf16x8, Aq[idx & 1][m][1]);
                            const bf16x8 b0 = __builtin_bit_cast(bf16x8, Bq[kx & 1][n + ky][0]), b1 = __builtin_bit_cast(bf16x8, Bq[kx & 1][n + ky][1]);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[m][n], 0, 0, 0);
                        } else if constexpr (F16) {
                            const f16x8 ah = __builtin_bit_cast(f16x8, Aq[idx & 1][m][0]), am = __builtin_bit_cast(f16x8, Aq[idx & 1][m][1]);
                            const f16x8 bh = __builtin_bit_cast(f16x8, Bq[kx & 1][n + ky][0]), bm = __builtin_bit_cast(f16x8, Bq[kx & 1][n + ky][1]);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(am, bh, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bm, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[m][n], 0, 0, 0);
                        } else {
                            const bf16x8 ah = __builtin_bit_cast(bf16x8, Aq[idx & 1][m][0]), am = __builtin_bit_cast(bf16x8, Aq[idx & 1][m][1]);
                            const bf16x8 bh = __builtin_bit_cast(bf16x8, Bq[kx & 1][n + ky][0]), bm = __builtin_bit_cast(bf16x8, Bq[kx & 1][n + ky][1]);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[m][n], 0, 0, 0);
                        }
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the next chunk's slots have landed ...
            __syncthreads();                                        // ... and every wave is done with this buffer
            buf ^= 1;
        }

#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] *= acc_scale;
        const auto [co0, tx, ty, b, y0, x0] = sp_tile(tile, a.coTiles, a.tilesX, a.tilesY);
        if constexpr (ST) {
            float* sc = reinterpret_cast<float*>(lds + 2 * BUF);       // [8 waves][64 channels][mean, M2]
            constexpr float npw = (float)(NT * 32), inv_npw = 1.f / npw;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int piv = __builtin_bit_cast(int, acc[m][0][r]);
                    const float p0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(piv, 0));
                    const float p1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(piv, 32));
                    const float pv = kh ? p1 : p0;
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const float d = acc[m][n][r] - pv;
                        s1 += d;
                        s2 = fmaf(d, d, s2);
                    }
                    s1 = sp_half_sum(s1);
                    s2 = sp_half_sum(s2);
                    if (l31 == 31) {
                        const int cl = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                        sc[(wn * 64 + cl) * 2] = fmaf(s1, inv_npw, pv);
                        sc[(wn * 64 + cl) * 2 + 1] = fmaxf(fmaf(-s1 * inv_npw, s1, s2), 0.f);
                    }
                }
            __syncthreads();
            if (tid < 64 && co0 + tid < a.Cout) {
                float mw[8], qw[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    mw[w] = sc[(w * 64 + tid) * 2];
                    qw[w] = sc[(w * 64 + tid) * 2 + 1];
                }
                const float mean = 0.125f * (((mw[0] + mw[1]) + (mw[2] + mw[3])) + ((mw[4] + mw[5]) + (mw[6] + mw[7])));
                float m2 = ((qw[0] + qw[1]) + (qw[2] + qw[3])) + ((qw[4] + qw[5]) + (qw[6] + qw[7]));
#pragma unroll
                for (int w = 0; w < 8; ++w) m2 = fmaf(npw * (mw[w] - mean), mw[w] - mean, m2);
                const int64_t nblk = (int64_t)a.B * a.tilesY * a.tilesX;
                const int64_t blk = ((int64_t)b * a.tilesY + ty) * a.tilesX + tx;
                float* sp = a.stats + ((int64_t)(co0 + tid) * nblk + blk) * 3;
                sp[0] = 8.f * npw;
                sp[1] = mean;
                sp[2] = m2;
            }
            __syncthreads();
        }
        float* zb = a.z + (int64_t)(W16 ? 2 * b + (l31 >> 4) : b) * a.z_bs;      // (W16: b is the image pair, lanes 16-31 hold the second image)
        const int xo = W16 ? (l31 & 15) : x0 + l31;
        // (PAIRS: a lane's image of the pair -- lanes 16-31 of a half-wave hold the second one, absent in the last tile of an odd count)
        [[maybe_unused]] const int img = PAIRS ? 2 * b + (l31 >> 4) : b;
        [[maybe_unused]] const bool img_ok = !PAIRS || img < a.n_img;
        if constexpr (ACT) {
            // BatchNorm (fixed coefficients) + ReLU on the accumulators, bn_relu_apply_split_kernel's expression; register r of
            // acc[m][n] is channel m 32 + 8 (r / 4) + 4 kh + r % 4 of the tile: four consecutive floats per coefficient and group
            const float* cf = act_cf + cf_par * 192;
            float vmax = 0.f;
            [[maybe_unused]] float vrow[NT];                      // RAG: the maximum per row n (the lane's pixel column is fixed)
            if constexpr (RAG) {
#pragma unroll
                for (int n = 0; n < NT; ++n) vrow[n] = 0.f;
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = m * 32 + 8 * g + 4 * kh;
                    const f32x4s mean = *reinterpret_cast<const f32x4s*>(cf + cl);
                    const f32x4s sc = *reinterpret_cast<const f32x4s*>(cf + 64 + cl);
                    const f32x4s sh = *reinterpret_cast<const f32x4s*>(cf + 128 + cl);
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float v = fmaxf(fmaf(acc[m][n][4 * g + j] - mean[j], sc[j], sh[j]), 0.f);
                            acc[m][n][4 * g + j] = v;
                            if constexpr (RAG) vrow[n] = fmaxf(vrow[n], v);
                            else vmax = fmaxf(vmax, v);
                        }
                }
            if constexpr (RAG) {
                // only the map's own pixels: one predicate per row (a.act_a's and the slot stores' guard; PAIRS: of real images only --
                // an absent image's accumulators are relu(sh - mean sc))
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    if (img_ok && y0 + wn * NT + n < a.H && xo < a.W) vmax = fmaxf(vmax, vrow[n]);
            }
            if (a.act_amax) {
                // the exact maximum of what this wave wrote: one atomicMax on the fp32 bit pattern per wave and tile
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
                if (lane == 0 && vmax == vmax)
                    atomicMax(a.act_amax + ((tile * NWV + wn) & (AMAX_SLOTS - 1)) * AMAX_STRIDE, __builtin_bit_cast(unsigned, vmax));
            }
            if (a.act_a) {
                float* ab = a.act_a + (int64_t)img * a.act_a_bs;
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const int yo = y0 + wn * NT + n;
                        if (img_ok && yo < a.H && xo < a.W) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                                if (co < a.Cout) ab[(int64_t)co * HW + (int64_t)yo * a.W + xo] = acc[m][n][r];
                            }
                        }
                    }
            }
        }
        if constexpr (PM == 1 && !ST && (!W16 || ACT)) {
            if (ACT || (a.zP && co0 >= a.zP_ch0)) {
                // Pre-split output (SpPreArgs::zP).  A lane holds channels 8 g + 4 kh + {0 .. 3} of its pixel for the four groups g of a
                // 32-row accumulator; v_permlane32_swap trades halves with the partner lane (kh ^ 1): afterwards a kh = 0 lane owns all
                // 8 channels of groups 0 and 2, a kh = 1 lane those of groups 1 and 3 -- whole slots, 512 contiguous bytes per half-wave
                const float zs = zP_scale;
                // (PAIRS: the slots go to the lane's image of the pair; the exchange partner, lane ^ 32, is in the same image half)
                u32x4s* zp = reinterpret_cast<u32x4s*>(reinterpret_cast<unsigned*>(a.zP) + (int64_t)img * a.zP_bs);
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const int yo = y0 + wn * NT + n;
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            float v[8];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                // (scalars first: __builtin_bit_cast applied to a vector ELEMENT yields element 0 with hipcc 7.2)
                                const float f0 = acc[m][n][8 * e + j], f1 = acc[m][n][8 * e + 4 + j];             // groups 2 e, 2 e + 1
                                const unsigned d0 = __builtin_bit_cast(unsigned, f0);
                                const unsigned d1 = __builtin_bit_cast(unsigned, f1);
                                const auto sw = __builtin_amdgcn_permlane32_swap(d0, d1, false, false);
                                const unsigned lo = sw[0], hi4 = sw[1];
                                v[j] = __builtin_bit_cast(float, lo);
                                v[4 + j] = __builtin_bit_cast(float, hi4);
                            }
                            u32x4s hi, mid;
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                unsigned hh, mm;
                                split2h_s(v[2 * k], v[2 * k + 1], zs, hh, mm);
                                hi[k] = hh;
                                mid[k] = mm;
                            }
                            if (img_ok && yo < a.H && xo < a.W) {
                                const int c8 = ((co0 - a.zP_ch0 + m * 32) >> 3) + 2 * e + kh;
                                u32x4s* d = zp + ((int64_t)(c8 * a.H + yo) * 2) * a.W + xo;
                                d[0] = hi;
                                d[a.W] = mid;
                            }
                        }
                    }
                if constexpr (POOL) {
                    // 2 x 2 max-pooling of the activation tile (SpPreArgs::pl_*): the window of pooled pixel (y0 / 2 + wn, (x0 + l31) / 2)
                    // is the lane's two rows n at its own pixel column and at the lane ^ 1 neighbour's -- an in-lane fmaxf, one quad-permute
                    // DPP step, and both lanes of a pair hold the maximum.  The slot form is the full-resolution one (permlane32 swap: all
                    // 8 channels of the pixel in one lane, the same 2^k); the even lanes store, 256 contiguous bytes per half-wave
                    const int Hp = a.H >> 1, Wp = a.W >> 1, yp = (y0 >> 1) + wn, xp = (x0 + l31) >> 1;
                    const bool pst = (l31 & 1) == 0 && yp < Hp && xp < Wp;
                    u32x4s* const yP = reinterpret_cast<u32x4s*>(reinterpret_cast<unsigned*>(a.pl_P) + (int64_t)b * a.pl_P_bs);
                    float* const yF = a.pl_y + (int64_t)b * a.pl_y_bs;
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            float v[8];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float t0 = acc[m][0][8 * e + j], u0 = acc[m][1][8 * e + j];                 // group 2 e: rows 0, 1
                                const float t1 = acc[m][0][8 * e + 4 + j], u1 = acc[m][1][8 * e + 4 + j];         // group 2 e + 1
                                const float f0 = dpp_max<0xB1>(fmaxf(t0, u0)), f1 = dpp_max<0xB1>(fmaxf(t1, u1)); // quad_perm [1,0,3,2]
                                if (a.pl_y && pst) {
                                    const int co = co0 + m * 32 + 16 * e + 4 * kh + j;
                                    yF[((int64_t)co * Hp + yp) * Wp + xp] = f0;
                                    yF[((int64_t)(co + 8) * Hp + yp) * Wp + xp] = f1;
                                }
                                const unsigned d0 = __builtin_bit_cast(unsigned, f0);
                                const unsigned d1 = __builtin_bit_cast(unsigned, f1);
                                const auto sw = __builtin_amdgcn_permlane32_swap(d0, d1, false, false);
                                const unsigned lo = sw[0], hi4 = sw[1];
                                v[j] = __builtin_bit_cast(float, lo);
                                v[4 + j] = __builtin_bit_cast(float, hi4);
                            }
                            u32x4s hi, mid;
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                unsigned hh, mm;
                                split2h_s(v[2 * k], v[2 * k + 1], zs, hh, mm);
                                hi[k] = hh;
                                mid[k] = mm;
                            }
                            if (a.pl_P && pst) {
                                const int c8 = ((co0 + m * 32) >> 3) + 2 * e + kh;
                                u32x4s* d = yP + ((int64_t)(c8 * Hp + yp) * 2) * Wp + xp;
                                d[0] = hi;
                                d[Wp] = mid;
                            }
                        }
                }
                continue;
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int yo = y0 + wn * NT + n;
                if (yo < a.H && xo < a.W) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                        if (co < a.Cout) zb[(int64_t)co * HW + (int64_t)yo * a.W + xo] = acc[m][n][r];
                    }
                }
            }
    }
}


// ------------------------------------------------------------------ the same tile on v_mfma_f32_16x16x32 (round 5)
// MI355X_MICROARCH.md, 'DVFS give-back' (7): in clock-limited MFMA loops the chip holds a higher clock on the 16x16x32 shape than on
// 32x32x16 at equal cycles per FLOP (half the accumulator traffic per FLOP).  Measured in this kernel (profiles/r05_mfma_shape_ab.md):
// the same matrix work issued as 16x16x32 runs 8-9 % faster on every layer shape.  So: the block, its LDS image (SpPreCfg) and the DMA
// schedule of conv3x3_split_pre_kernel and the family's persistent tile walk (sp_tile_range, sp_tile), with the wave's 64 channels
// x 2 rows x 32 pixels held as SIXTEEN 16 x 16
// accumulators, M = 16 pixels of a row (A = input fragment), N = 16 output channels (B = weight fragment): a lane then owns four
// CONSECUTIVE pixels of one channel -- the epilogue stores float4s (16 store instructions per wave and tile instead of 64) and the
// BatchNorm statistics need in-lane sums plus two cross-lane steps per channel tile (the 32x32 form: 5 DPP steps per register).
// K = 32 per instruction:
//  * PM == 2 (plain bf16, 32-channel chunks): K = the chunk's 32 channels -- lane group q = lane / 16 reads channel group q.  Nine
//    steps of 16 MFMAs per chunk, the fragment reads of the 32x32 form (36 weight + 24 input per wave and chunk).
//  * split operands (16-channel chunks, three product terms per tap): K-packing.
//      'a' step (tap):          A = [x_hi | x_hi]            B = [w_hi(tap) | w_mid(tap)]      -> x_hi w_hi + x_hi w_mid
//      'H' step (ky), taps (ky,0), (ky,1):  A = [x_mid(kx=0) | x_mid(kx=1)]  B = [w_hi(ky,0) | w_hi(ky,1)]
//      'V' step, taps (0,2), (1,2):         A = [x_mid(row n) | x_mid(row n+1)] at kx = 2,  B = [w_hi(0,2) | w_hi(1,2)]
//      'S' step, tap (2,2):                 A = [x_mid(row n+2) | same],  B = [w_hi(2,2) | 0]   (27 K16 products are an odd number:
//    one half instruction per tile and chunk is padding -- 14 steps for 13.5 steps' worth, +3.7 %; the zero half reads the zero padding
//    behind the halo image).  Lanes pick their K group by address: every fragment is still ONE conflict-free ds_read_b128.
//
// ACT (eval-mode inference on plain bf16 operands): conv3x3_split_pre_kernel's activation epilogue in this lane layout -- the fixed
// BatchNorm + ReLU of SpPreArgs::act_* on the accumulators, every channel out through the one-part slot store (zP, zP_ch0 = 0, unscaled:
// bf16 has fp32's exponent range, there is no guard), z never written.
//
// HEAD (labels-only inference, the model's last unit: Cout == 64, so a block's one channel tile holds every output channel of its
// pixels): the same activation on the accumulators, then the head's product with L (SpPreArgs::hd_*) summed over the channels --
// in-lane over the four channel tiles, four DPP steps over the 16 channel lanes of a row -- and V [B][H][W] as the ONLY store: neither
// z nor an activation leaves the kernel.  No LDS traffic beyond the coefficients, no atomics, a fixed order: deterministic.
template <int CTRL> __device__ __forceinline__ float dpp_add(float x) {     // x + (x of the lane DPP control CTRL selects)
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
// The one-part bf16 slot form of conv3x3_pre16_kernel's accumulator layout: the eight lanes c8 = 0 .. 7 of a group hold 8 channels x 4
// pixels of channel group A (d1: the lane's channel c8 of A at four pixels) and of group B (d2).  Three butterfly exchanges (lane ^ 1,
// ^ 2, ^ 4) transpose them: afterwards lane c8 owns one whole 16-byte slot -- the 8 channels of group (c8 >> 2 ? B : A) at pixel c8 & 3.
__device__ __forceinline__ u32x4s pre16_slot_transpose(const f32x4s& d1, const f32x4s& d2, int c8) {
    const unsigned a0 = pack2bf(d1[0], d1[1]), a1 = pack2bf(d1[2], d1[3]);
    const unsigned b0 = pack2bf(d2[0], d2[1]), b1 = pack2bf(d2[2], d2[3]);
    const bool o1 = (c8 & 1) != 0, o2 = (c8 & 2) != 0, o4 = (c8 & 4) != 0;
    // stage 1: (pixel pair of one channel) x 2 lanes -> (channel pair) of pixel (c8 & 1) [and + 2]
    auto st1 = [&](unsigned x) {
        const unsigned y = (unsigned)__shfl_xor((int)x, 1, 64);
        return o1 ? ((y >> 16) | (x & 0xffff0000u)) : ((x & 0xffffu) | (y << 16));
    };
    const unsigned A0 = st1(a0), A1 = st1(a1), B0 = st1(b0), B1 = st1(b1);
    // stage 2: -> the channel quad (c8 >> 2) of pixel c8 & 3: lanes with bit 1 clear keep pixel (c8 & 1), the others + 2
    const unsigned ra = (unsigned)__shfl_xor((int)(o2 ? A0 : A1), 2, 64), rb = (unsigned)__shfl_xor((int)(o2 ? B0 : B1), 2, 64);
    const unsigned ka = o2 ? A1 : A0, kb = o2 ? B1 : B0;
    const unsigned Alo = o2 ? ra : ka, Ahi = o2 ? ka : ra, Blo = o2 ? rb : kb, Bhi = o2 ? kb : rb;
    // stage 3: lanes with bit 2 clear collect group A (their quad = channels 0 .. 3, the partner's 4 .. 7), the others B
    const unsigned r0 = (unsigned)__shfl_xor((int)(o4 ? Alo : Blo), 4, 64), r1 = (unsigned)__shfl_xor((int)(o4 ? Ahi : Bhi), 4, 64);
    return o4 ? u32x4s{r0, r1, Blo, Bhi} : u32x4s{Alo, Ahi, r0, r1};
}
// RAG (round 13, the ragged entries): the pooled fp32 store on maps that are not made of full tiles.  Everything else of the kernel
// already is per-slot / per-float4 bounds-checked (staging: the out-of-range offset; stores: yo < H && xo < W), so the ragged entries
// launch the full-tile instances; only the pooled fp32 rows, whose two float2 per lane share ONE guard on full tiles, need code.
// ANY (round 15, the entries of include/onet_hip_anymap.h): the activation epilogue's two fp32 side outputs on maps of ANY H and W --
// rows of W floats are not 16-byte aligned at W = 25 or 50, and an odd map ends in the middle of a float4 / a pooled float2 -- stored
// float by float, each under its own guard.  Pooling is floor pooling (Hp = H >> 1, Wp = W >> 1): a 2 x 2 window that is only partly
// inside an odd map has a pooled index >= Hp / Wp, so the guards on pooled coordinates keep it out of every pooled store.  Staging,
// main loop and slot stores are the other instances': per slot, at any width.
template <bool ST, int PM, bool W16, bool RD = false, bool ACT = false, bool HEAD = false, bool POOL = false, bool RAG = false, bool ANY = false>
__global__ __launch_bounds__(512, 2) void conv3x3_pre16_kernel(SpPreArgs a) {
    constexpr bool F16 = PM == 1;
    static_assert(!ANY || (ACT && PM == 2 && !RAG), "conv3x3_pre16_kernel: the any-map instance is the one-part activation epilogue's");
    static_assert(!POOL || ACT, "conv3x3_pre16_kernel: the pooled stores ride on the activation epilogue");
    static_assert(!RAG || (POOL && PM == 2), "conv3x3_pre16_kernel: the ragged instance is the one-part pooled epilogue's");
    static_assert(!ACT || (PM == 2 && !ST && !RD && (!W16 || !(POOL || RAG || ANY))),
                  "conv3x3_pre16_kernel: the activation epilogue goes with the one-part bf16 slot store; on image-pair tiles: no pooled, ragged or any-map twin");
    static_assert(!HEAD || (PM != 0 && !ST && !W16 && !RD && !ACT), "conv3x3_pre16_kernel: the head epilogue replaces every store of a plain forward launch");
    using C = SpPreCfg<W16>;
    static_assert(C::NW == 8 && C::NT == 2, "conv3x3_pre16_kernel: 8 waves of 2 rows");
    constexpr int NT = 2, IN_COLS = C::IN_COLS, NWI = C::NWI, CO_T = C::CO_T, NPIXP = C::NPIXP;
    constexpr int BUF = C::BUF_SLOTS, IN_PART = C::IN_PART;
    constexpr int NII = (2 * IN_PART + 511) / 512;
    constexpr int CH_OFF = W16 ? 18 : 16;                              // column of the second 16-pixel tile in the halo image
    constexpr int NSTEP = PM == 2 ? 9 : 14;
    constexpr bool PAIRS = W16 && ACT;                                 // the activation epilogue on image-pair tiles (SpPreArgs::n_img)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    u32x4s* lds = reinterpret_cast<u32x4s*>(smem_s);

    int t_first, t_end, t_stride;                                      // tile list order: see sp_tile_range
    sp_tile_range(a.tilesX * a.tilesY * a.B * a.coTiles, t_first, t_end, t_stride);
    if (t_first >= t_end) return;

    const int tid = threadIdx.x, lane = tid & 63, wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, lq = lane >> 4, hq = lq & 1, gq = lq >> 1;
    const int HW = a.H * a.W;
    const int nchunks = PM == 2 ? a.Cin >> 5 : a.Cin >> 4;

    const i32x4s wr = sp_rsrc4(a.wq, (int64_t)a.Cin * (PM == 2 ? 1 : 2) * 9 * a.Cout * 2);
    float xs_inv = 1.f, xs_inv2 = 1.f;
    (void)amax_scale(amax_read(a.x_slots), a.x_always != 0, xs_inv);
    (void)amax_scale(amax_read(a.x_slots2), a.x_always != 0, xs_inv2);
    const int split_chunk = a.split_ch ? (PM == 2 ? a.split_ch >> 5 : a.split_ch >> 4) : 0;
    const float grp_ratio = split_chunk ? xs_inv / xs_inv2 : 1.f;
    const float acc_scale = (split_chunk ? xs_inv2 : xs_inv) * (F16 ? reinterpret_cast<const float*>(a.wq + (int64_t)a.Cin * 2 * 9 * a.Cout)[1] : 1.f);
    const unsigned in_step = (unsigned)(16 * HW * 4), w_step = (unsigned)(2 * 9 * 2 * a.Cout * 16);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_s;

    // ---- staging (conv3x3_split_pre_kernel's): slot position i = (wn + 8 k) * 64 + lane of the chunk image
    unsigned in_off[NII], w_off[NWI];
    i32x4s xr;
    int st_tile = t_first, st_chunk = 0;
    unsigned cin_bytes = 0, cw_bytes = 0;
    auto setup_stage = [&]() __attribute__((always_inline)) {
        const bool live = st_tile < t_end;
        const auto [co0, tx, ty, b, y0, x0] = sp_tile(live ? st_tile : t_first, a.coTiles, a.tilesX, a.tilesY);
        // (PAIRS: the last tile of an odd image count holds one image -- the resource ends with it, its second half is out of range)
        const bool img1 = !PAIRS || 2 * b + 1 < a.n_img;
        xr = sp_rsrc4(reinterpret_cast<const unsigned*>(a.xs) + (int64_t)(W16 ? 2 * b : b) * a.xs_bs,
                      (W16 && img1 ? a.xs_bs * 4 : 0) + (int64_t)a.Cin * HW * (PM == 2 ? 2 : 4));
#pragma unroll
        for (int k = 0; k < NII; ++k) {
            const int i = (wn + 8 * k) * 64 + lane;
            const int ph = i / NPIXP, pix = i % NPIXP;
            const int r = pix / IN_COLS, c = pix % IN_COLS;
            const int img = W16 ? c / 18 : 0;
            const int yy = y0 - 1 + r, xx = W16 ? c % 18 - 1 : x0 - 1 + c;
            const bool ok = live && i < 2 * IN_PART && pix < C::NPIX && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W && (!PAIRS || img == 0 || img1);
            const unsigned io = W16 ? (unsigned)(img * a.xs_bs * 4) : 0u;
            in_off[k] = !ok ? OOB_S : PM == 2 ? io + (unsigned)(((ph * a.H + yy) * a.W + xx) * 16)
                                              : io + (unsigned)(((((ph & 1) * a.H + yy) * 2 + (ph >> 1)) * a.W + xx) * 16);
        }
#pragma unroll
        for (int k = 0; k < NWI; ++k) {
            const int i = tid + 512 * k;
            const int co = i & (CO_T - 1), pth = i >> 6;
            const bool ok = live && (i < C::W_SLOTS) && (co0 + co < a.Cout);
            w_off[k] = ok ? (unsigned)((pth * a.Cout + co0 + co) * 16) : OOB_S;
        }
    };
    auto advance = [&]() __attribute__((always_inline)) {
        ++st_chunk;
        cin_bytes += in_step;
        cw_bytes += w_step;
        if (st_chunk == nchunks) {
            st_chunk = 0;
            cin_bytes = cw_bytes = 0;
            st_tile += t_stride;
            setup_stage();
        }
    };
    auto dma_in = [&](int buf, int k) __attribute__((always_inline)) {
        if ((wn + 8 * k) * 64 < 2 * IN_PART)
            sp_dma16(xr, lds0 + (unsigned)((buf * BUF + C::W_SLOTS + (wn + 8 * k) * 64) * 16), in_off[k], cin_bytes);
    };
    auto dma_w = [&](int buf, int k) __attribute__((always_inline)) {
        if (k < NWI - 1 || wn < (C::W_SLOTS - 512 * (NWI - 1)) / 64)
            sp_dma16(wr, lds0 + (unsigned)((buf * BUF + (wn + 8 * k) * 64) * 16), w_off[k], cw_bytes);
    };

    // ---- fragment bases (slots inside a chunk buffer).  Lane (r16, lq): row / column r16 of the 16 x 16 tile, K group lq (8 values)
    const int xrow0 = (wn * NT) * IN_COLS + r16;
    const u32x4s* const xa_p = lds + C::W_SLOTS + (PM == 2 ? lq : hq) * NPIXP + xrow0;        // + row * IN_COLS + ch * CH_OFF + kx
    const u32x4s* const xh_p = lds + C::W_SLOTS + (2 + hq) * NPIXP + xrow0 + gq;                // 'H': x_mid, kx = gq
    const u32x4s* const xv_p = lds + C::W_SLOTS + (2 + hq) * NPIXP + xrow0 + gq * IN_COLS + 2;  // 'V': x_mid, rows n + gq, kx = 2
    const u32x4s* const xs_p = lds + C::W_SLOTS + (2 + hq) * NPIXP + xrow0 + 2;                 // 'S': x_mid, kx = 2 (both K halves)
    const u32x4s* const wa_p = lds + (gq * 9 * 2 + hq) * CO_T + r16;                            // + tap * 2 CO_T + ct * 16: [w_hi | w_mid] (PM 2: 32 channels)
    const u32x4s* const wh_p = lds + (gq * 2 + hq) * CO_T + r16;                                // 'H': + ky * 6 CO_T + ct * 16: taps (ky, gq)
    const u32x4s* const wv_p = lds + ((3 * gq + 2) * 2 + hq) * CO_T + r16;                      // 'V': taps (gq, 2)
    const u32x4s* const ws_p = gq == 0 ? lds + (8 * 2 + hq) * CO_T + r16 : lds + C::W_SLOTS + C::NPIX;   // 'S': tap (2,2) | zeros
    const int ws_ct = gq == 0 ? 16 : 0;

    setup_stage();
#pragma unroll
    for (int k = 0; k < NII; ++k) dma_in(0, k);
#pragma unroll
    for (int k = 0; k < NWI; ++k) dma_w(0, k);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    // ACT: the tile's 64 x (mean, sc, sh) in LDS behind the chunk buffers, [tile parity][3][64] floats, fetched one tile ahead and
    // committed at the top of the tile (conv3x3_split_pre_kernel's act_fetch / act_cf: a wave still in the previous tile's epilogue
    // reads the other copy, and nobody gets two tiles ahead of a chunk barrier)
    [[maybe_unused]] float* const act_cf = reinterpret_cast<float*>(lds + 2 * BUF);
    [[maybe_unused]] float cf_next = 0.f;
    [[maybe_unused]] int cf_par = 0;
    auto act_fetch = [&](int t) __attribute__((always_inline)) {
        if (tid < 192 && t < t_end) {
            const int k = tid >> 6;                                 // 0: mean, 1: sc, 2: sh   (save rows 0, 2, 3)
            cf_next = a.act_save[(int64_t)(k + (k > 0)) * a.Cout + sp_tile(t, a.coTiles, a.tilesX, a.tilesY).co0 + (tid & 63)];
        }
    };
    if constexpr (ACT || HEAD) act_fetch(t_first);
    for (int tile = t_first; tile < t_end; tile += t_stride) {
        if constexpr (ACT || HEAD) {
            cf_par ^= 1;
            if (tid < 192) act_cf[cf_par * 192 + tid] = cf_next;
            act_fetch(tile + t_stride);
        }
        f32x4s acc[4][NT][2];                       // [channel tile][row][16-pixel tile]
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) acc[ct][n][ch] = f32x4s{0.f, 0.f, 0.f, 0.f};

        for (int c = 0; c < nchunks; ++c) {
            if (split_chunk && c == split_chunk && grp_ratio != 1.f) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int ch = 0; ch < 2; ++ch) acc[ct][n][ch] *= grp_ratio;
            }
            const int bo = buf * BUF;
            u32x4s Xp[2][NT + 2][2], Wf[2][4];
            // the input fragments of pool p for phase ph (0..2: 'a' at kx = ph; 3: 'H'; 4: 'V' rows 0..1 + 'S' rows 2..3), fragment f
            auto load_x = [&](int ph, int f) __attribute__((always_inline)) {
                const int j = f >> 1, ch = f & 1, p = ph & 1;
                if (ph < 3) Xp[p][j][ch] = xa_p[bo + j * IN_COLS + ch * CH_OFF + ph];
                else if (ph == 3) Xp[p][j][ch] = xh_p[bo + j * IN_COLS + ch * CH_OFF];
                else if (j < NT) Xp[p][j][ch] = xv_p[bo + j * IN_COLS + ch * CH_OFF];
                else Xp[p][j][ch] = xs_p[bo + j * IN_COLS + ch * CH_OFF];
            };
            auto load_w = [&](int s) __attribute__((always_inline)) {       // the weight fragments of step s
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (s < 9) Wf[s & 1][ct] = wa_p[bo + ((s % 3) * 3 + s / 3) * 2 * CO_T + ct * 16];
                    else if (s < 12) Wf[s & 1][ct] = wh_p[bo + (s - 9) * 6 * CO_T + ct * 16];
                    else if (s == 12) Wf[s & 1][ct] = wv_p[bo + ct * 16];
                    else Wf[s & 1][ct] = ws_p[bo + ct * ws_ct];
                }
            };
#pragma unroll
            for (int f = 0; f < 2 * (NT + 2); ++f) load_x(0, f);
            load_w(0);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                const int ph = s < 9 ? s / 3 : (s < 12 ? 3 : 4);           // phase of this step; its fragments sit in pool ph & 1
                const int ro = s < 9 ? s % 3 : (s < 12 ? s - 9 : (s == 12 ? 0 : NT));   // first fragment row of output row 0
                if (s + 1 < NSTEP) load_w(s + 1);
                if (s < 12 && ph + 1 < (PM == 2 ? 3 : 5)) {                // the next phase's input fragments, a third per step
#pragma unroll
                    for (int f = 0; f < 2 * (NT + 2); ++f)
                        if (f % 3 == s % 3) load_x(ph + 1, f);
                }
                if (s == 0) advance();
                {
                    constexpr int NPIECE = NII + NWI, PER = (NPIECE + C::LAST_TAP) / (C::LAST_TAP + 1);
#pragma unroll
                    for (int q = 0; q < PER; ++q) {
                        const int pc = s * PER + q;
                        if (s <= C::LAST_TAP && pc < NPIECE) {
                            if (pc & 1) { if (pc / 2 < NWI) dma_w(buf ^ 1, pc / 2); else dma_in(buf ^ 1, pc - NWI); }
                            else { if (pc / 2 < NII) dma_in(buf ^ 1, pc / 2); else dma_w(buf ^ 1, pc - NII); }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int ch = 0; ch < 2; ++ch) {
                            if constexpr (F16)
                                acc[ct][n][ch] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, Xp[ph & 1][ro + n][ch]),
                                                                                        __builtin_bit_cast(f16x8, Wf[s & 1][ct]), acc[ct][n][ch], 0, 0, 0);
                            else
                                acc[ct][n][ch] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, Xp[ph & 1][ro + n][ch]),
                                                                                         __builtin_bit_cast(bf16x8, Wf[s & 1][ct]), acc[ct][n][ch], 0, 0, 0);
                        }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            buf ^= 1;
        }

#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) acc[ct][n][ch] *= acc_scale;
        const auto [co0, tx, ty, b, y0, x0] = sp_tile(tile, a.coTiles, a.tilesX, a.tilesY);
        if constexpr (ST) {
            // BatchNorm (n, mean, M2) record of the tile per channel.  Lane = channel r16 of tile ct, 16 pixel values in registers:
            // own pivot-shifted sums -> (mean, M2) of 16; the four lane groups merged pairwise (equal counts: Chan's formula); the
            // eight waves through LDS -- in the chunk buffer nobody reads until the next chunk's DMA (issued behind the barriers below)
            float* sc = reinterpret_cast<float*>(lds + (buf ^ 1) * BUF);       // [8 waves][64 channels][mean, M2]
            constexpr float npw = (float)(NT * 32);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const float pv = acc[ct][0][0][0];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float d = acc[ct][n][ch][r] - pv;
                            s1 += d;
                            s2 = fmaf(d, d, s2);
                        }
                float mean = fmaf(s1, 1.f / 16.f, pv), m2 = fmaxf(fmaf(-s1 * (1.f / 16.f), s1, s2), 0.f), cnt = 16.f;
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    const float mo = __shfl_xor(mean, o, 64), qo = __shfl_xor(m2, o, 64);
                    const float dlt = mo - mean;
                    m2 = (m2 + qo) + (0.5f * cnt) * dlt * dlt;
                    mean = 0.5f * (mean + mo);
                    cnt *= 2.f;
                }
                if (lq == 0) {
                    sc[(wn * 64 + ct * 16 + r16) * 2] = mean;
                    sc[(wn * 64 + ct * 16 + r16) * 2 + 1] = m2;
                }
            }
            __syncthreads();
            if (tid < 64 && co0 + tid < a.Cout) {
                float mw[8], qw[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    mw[w] = sc[(w * 64 + tid) * 2];
                    qw[w] = sc[(w * 64 + tid) * 2 + 1];
                }
                const float mean = 0.125f * (((mw[0] + mw[1]) + (mw[2] + mw[3])) + ((mw[4] + mw[5]) + (mw[6] + mw[7])));
                float m2 = ((qw[0] + qw[1]) + (qw[2] + qw[3])) + ((qw[4] + qw[5]) + (qw[6] + qw[7]));
#pragma unroll
                for (int w = 0; w < 8; ++w) m2 = fmaf(npw * (mw[w] - mean), mw[w] - mean, m2);
                const int64_t nblk = (int64_t)a.B * a.tilesY * a.tilesX;
                const int64_t blk = ((int64_t)b * a.tilesY + ty) * a.tilesX + tx;
                float* sp = a.stats + ((int64_t)(co0 + tid) * nblk + blk) * 3;
                sp[0] = 8.f * npw;
                sp[1] = mean;
                sp[2] = m2;
            }
            __syncthreads();
        }
        if constexpr (ACT) {
            // BatchNorm (fixed coefficients) + ReLU on the accumulators, bn_relu_apply_split_kernel's expression: the lane's channel of
            // channel tile ct is 16 ct + r16 -- one (mean, sc, sh) per channel tile
            const float* cf = act_cf + cf_par * 192;
            float vmax = 0.f;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const float mean = cf[ct * 16 + r16], sc = cf[64 + ct * 16 + r16], sh = cf[128 + ct * 16 + r16];
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float v = fmaxf(fmaf(acc[ct][n][ch][r] - mean, sc, sh), 0.f);
                            acc[ct][n][ch][r] = v;
                            vmax = fmaxf(vmax, v);
                        }
            }
            if (a.act_amax) {
                // the exact maximum of what this wave wrote (bf16 rounding is monotone: the slots' maximum is bf16 of it): one atomicMax
                // on the fp32 bit pattern per wave and tile
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
                if (lane == 0 && vmax == vmax)
                    atomicMax(a.act_amax + ((tile * 8 + wn) & (AMAX_SLOTS - 1)) * AMAX_STRIDE, __builtin_bit_cast(unsigned, vmax));
            }
        }
        if constexpr (HEAD) {
            // The L tile in the accumulator layout (RD's z loads: the lane's channel 16 ct + r16 at pixels 4 lq .. + 3 of both 16-pixel
            // halves of its two rows) goes into registers first; the main loop's fragment registers are dead here
            f32x4s lr[4][NT][2];
            const float* Lb = a.hd_L + (int64_t)b * a.hd_L_bs;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        const int co = co0 + ct * 16 + r16, yo = y0 + wn * NT + n, xo = x0 + 16 * ch + 4 * lq;
                        f32x4s ll = {0.f, 0.f, 0.f, 0.f};
                        if (co < a.Cout && yo < a.H && xo < a.W) ll = *reinterpret_cast<const f32x4s*>(Lb + (int64_t)co * HW + (int64_t)yo * a.W + xo);
                        lr[ct][n][ch] = ll;
                    }
            __builtin_amdgcn_sched_barrier(0);
            // h = relu(bn(acc)) by head_softmax_fwd_kernel's expression, v += L h: the channel tiles in order, one fmaf chain per pixel
            const float* cf = act_cf + cf_par * 192;
            f32x4s v[NT][2];
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) v[n][ch] = f32x4s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const float mean = cf[ct * 16 + r16], sc = cf[64 + ct * 16 + r16], sh = cf[128 + ct * 16 + r16];
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            v[n][ch][r] = fmaf(lr[ct][n][ch][r], fmaxf(fmaf(acc[ct][n][ch][r] - mean, sc, sh), 0.f), v[n][ch][r]);
            }
            // the 16 channel lanes r16 of a DPP row: lane ^ 1, lane ^ 2 (quad permutes), then the quads of a half and the halves of the
            // row by the mirror modes -- below each step the sums are equal in the lanes it pairs, so every lane ends with the same bits
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        v[n][ch][r] = dpp_add<0x140>(dpp_add<0x141>(dpp_add<0x4E>(dpp_add<0xB1>(v[n][ch][r]))));   // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
            // one lane per (row, half, pixel quad) stores: lane r16 = 2 n + ch, so the wave's 16 float4s leave as four 64-byte runs
            float* Vb = a.hd_V + (int64_t)b * HW;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const int yo = y0 + wn * NT + n, xo = x0 + 16 * ch + 4 * lq;
                    if (r16 == 2 * n + ch && yo < a.H && xo < a.W) *reinterpret_cast<f32x4s*>(Vb + (int64_t)yo * a.W + xo) = v[n][ch];
                }
            continue;
        }
        // RD, part 1: the z tile of the unit below goes into registers FIRST (16 loads in flight; the fragment registers of the main loop
        // are dead here), the da stores below run while they travel, and the sums are taken after the stores
        f32x4s zr[4][NT][2];
        const float* rd_sv = nullptr;
        if constexpr (RD) {
            const int img0 = W16 ? 2 * b : b;
            rd_sv = a.rd_save + (int64_t)(a.rd_gimg ? img0 / a.rd_gimg : 0) * 4 * a.Cout;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        const int co = co0 + ct * 16 + r16, yo = y0 + wn * NT + n, xo = (W16 ? 0 : x0 + 16 * ch) + 4 * lq;
                        f32x4s zz = {0.f, 0.f, 0.f, 0.f};
                        if (co < a.Cout && yo < a.H && xo < a.W) {
                            const int64_t zo = (int64_t)(W16 ? img0 + ch : img0) * a.rd_z_bs + (int64_t)co * HW + (int64_t)yo * a.W + xo;
                            if (a.rd_z16) {
                                const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __bf16*>(a.rd_z) + zo);
                                zz = f32x4s{__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                                            __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
                            } else {
                                zz = *reinterpret_cast<const f32x4s*>(a.rd_z + zo);
                            }
                        }
                        zr[ct][n][ch] = zz;
                    }
            __builtin_amdgcn_sched_barrier(0);
        }
        // A lane holds, per (channel tile, row), channel r16's pixels 4 lq .. + 3 of BOTH 16-pixel tiles: stored as they stand, an
        // instruction would write 64-byte half lines (16 channels x 4 lanes x 16 B).  Lanes r16 >= 8 of the first tile and lanes
        // r16 < 8 of the second trade places (two masked row_ror:8 DPP moves per register) so that each store instruction writes
        // eight channels' WHOLE 128-byte lines: instruction 1 channels 0-7 (pixels 0-15 from lanes r16 < 8, 16-31 from lanes r16 >= 8),
        // instruction 2 channels 8-15.
        {
            const int half = r16 >> 3, c8 = r16 & 7;
            float* zb = a.z + (int64_t)(W16 ? 2 * b + half : b) * a.z_bs;      // (W16: the second 16-pixel tile is the pair's second image)
            const int xo = (W16 ? 0 : x0 + 16 * half) + 4 * lq;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int yo = y0 + wn * NT + n;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const i32x4s va = __builtin_bit_cast(i32x4s, acc[ct][n][0]), vb = __builtin_bit_cast(i32x4s, acc[ct][n][1]);
                    // d1: lanes 8-15 <- tile 1 of channel r16 - 8;  d2: lanes 0-7 <- tile 0 of channel r16 + 8
                    const i32x4s e1 = {__builtin_amdgcn_update_dpp(va.x, vb.x, 0x128, 0xf, 0xc, false), __builtin_amdgcn_update_dpp(va.y, vb.y, 0x128, 0xf, 0xc, false),
                                       __builtin_amdgcn_update_dpp(va.z, vb.z, 0x128, 0xf, 0xc, false), __builtin_amdgcn_update_dpp(va.w, vb.w, 0x128, 0xf, 0xc, false)};
                    const i32x4s e2 = {__builtin_amdgcn_update_dpp(vb.x, va.x, 0x128, 0xf, 0x3, false), __builtin_amdgcn_update_dpp(vb.y, va.y, 0x128, 0xf, 0x3, false),
                                       __builtin_amdgcn_update_dpp(vb.z, va.z, 0x128, 0xf, 0x3, false), __builtin_amdgcn_update_dpp(vb.w, va.w, 0x128, 0xf, 0x3, false)};
                    const f32x4s d1 = __builtin_bit_cast(f32x4s, e1), d2 = __builtin_bit_cast(f32x4s, e2);
                    if constexpr (PM == 2 && !ST && (!W16 || ACT) && !RD) {
                        // (PAIRS: after the exchange a lane's half IS the image of the pair -- d1, d2 hold that image's pixels 4 lq .. + 3)
                        const int img = PAIRS ? 2 * b + half : b;
                        const bool img_ok = !PAIRS || img < a.n_img;
                        if constexpr (ACT) {
                            // the activation in fp32 NCHW too, for a reader that takes no slots: the plain z store's float4s
                            if constexpr (ANY || PAIRS) {
                                // no row alignment, and the map may end inside the lane's four pixels: one guard per float (PAIRS: the
                                // accumulators at columns W .. 15 of a half are relu(bn(partial sums)), not zero)
                                if (a.act_a && img_ok && yo < a.H && xo < a.W) {
                                    const int co = co0 + ct * 16 + c8;
                                    float* o = a.act_a + (int64_t)img * a.act_a_bs + (int64_t)co * HW + (int64_t)yo * a.W + xo;
#pragma unroll
                                    for (int i = 0; i < 4; ++i)
                                        if (xo + i < a.W) {
                                            if (co < a.Cout) o[i] = d1[i];
                                            if (co + 8 < a.Cout) o[(int64_t)8 * HW + i] = d2[i];
                                        }
                                }
                            } else if (a.act_a && yo < a.H && xo < a.W) {
                                const int co = co0 + ct * 16 + c8;
                                float* o = a.act_a + (int64_t)b * a.act_a_bs + (int64_t)co * HW + (int64_t)yo * a.W + xo;
                                if (co < a.Cout) *reinterpret_cast<f32x4s*>(o) = d1;
                                if (co + 8 < a.Cout) *reinterpret_cast<f32x4s*>(o + (int64_t)8 * HW) = d2;
                            }
                        }
                        if (ACT || (a.zP && co0 >= a.zP_ch0)) {
                            // Pre-split output, plain bf16 (SpPreArgs::zP, one part): channel group A = d1 (channels 16 ct + c8), group B =
                            // d2 (+ 8) through pre16_slot_transpose -- lane c8 then owns the slot of group (c8 >> 2 ? B : A) at pixel c8 & 3
                            const bool o4 = (c8 & 4) != 0;
                            const u32x4s slot = pre16_slot_transpose(d1, d2, c8);
                            const int xs = (PAIRS ? 0 : x0 + 16 * half) + 4 * lq + (c8 & 3);
                            if (img_ok && yo < a.H && xs < a.W) {
                                const int g8 = ((co0 - a.zP_ch0) >> 3) + 2 * ct + (o4 ? 1 : 0);
                                u32x4s* zp = reinterpret_cast<u32x4s*>(reinterpret_cast<unsigned*>(a.zP) + (int64_t)img * a.zP_bs);
                                zp[((int64_t)g8 * a.H + yo) * a.W + xs] = slot;
                            }
                            continue;
                        }
                    }
                    if (yo < a.H && xo < a.W) {
                        const int co = co0 + ct * 16 + c8;
                        const int64_t off = (int64_t)co * HW + (int64_t)yo * a.W + xo;
                        if (a.z16) {          // z stored as bf16: 8 bytes per lane, 64 contiguous bytes per channel row and instruction
                            __bf16* o = reinterpret_cast<__bf16*>(a.z) + (int64_t)(W16 ? 2 * b + half : b) * a.z_bs + off;
                            const bf16x2 p0 = {(__bf16)d1[0], (__bf16)d1[1]}, p1 = {(__bf16)d1[2], (__bf16)d1[3]};
                            const bf16x2 q0 = {(__bf16)d2[0], (__bf16)d2[1]}, q1 = {(__bf16)d2[2], (__bf16)d2[3]};
                            if (co < a.Cout) *reinterpret_cast<uint2*>(o) = uint2{__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1)};
                            if (co + 8 < a.Cout) *reinterpret_cast<uint2*>(o + (int64_t)8 * HW) = uint2{__builtin_bit_cast(unsigned, q0), __builtin_bit_cast(unsigned, q1)};
                        } else {
                            float* o = zb + off;
                            if (co < a.Cout) *reinterpret_cast<f32x4s*>(o) = d1;
                            if (co + 8 < a.Cout) *reinterpret_cast<f32x4s*>(o + (int64_t)8 * HW) = d2;
                        }
                    }
                }
            }
        }
        if constexpr (POOL) {
            // 2 x 2 max-pooling of the activation tile (SpPreArgs::pl_*).  The lane holds channel 16 ct + r16 at pixels 4 lq .. + 3 of both
            // 16-pixel halves of its two rows: two windows per half, all in the lane -- pooled pixels 2 lq, 2 lq + 1 and 8 + 2 lq, 8 + 2 lq + 1
            // of the tile's 16, row y0 / 2 + wn.  Slots: the butterfly of the full-resolution store with channel tiles 2 p and 2 p + 1 as
            // its groups A and B -- lane c8 of a half (r16 >> 3: channels + 8) then owns all 8 channels of one pooled pixel, and two
            // store instructions per wave and tile write whole 16-byte slots, 256 contiguous bytes per channel group
            const int Hp = a.H >> 1, Wp = a.W >> 1, yp = (y0 >> 1) + wn, xp0 = (x0 >> 1) + 2 * lq;
            f32x4s pm[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const f32x4s t = acc[ct][0][ch], u = acc[ct][1][ch];
                    pm[ct][2 * ch] = fmaxf(fmaxf(t[0], t[1]), fmaxf(u[0], u[1]));
                    pm[ct][2 * ch + 1] = fmaxf(fmaxf(t[2], t[3]), fmaxf(u[2], u[3]));
                }
            if constexpr (ANY) {
                // one guard per float: Wp may be odd and the pooled rows are not 8-byte aligned; the address is formed under the guard
                if (a.pl_y && yp < Hp) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int co = co0 + ct * 16 + r16;
                        if (co < a.Cout) {
                            float* row = a.pl_y + (int64_t)b * a.pl_y_bs + ((int64_t)co * Hp + yp) * Wp;
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int xp = xp0 + (i & 1) + (i & 2 ? 8 : 0);
                                if (xp < Wp) row[xp] = pm[ct][i];
                            }
                        }
                    }
                }
            } else if constexpr (RAG) {
                // one guard per float2: Wp and xp0 are even (W % 4 == 0), so a pair is wholly inside the pooled row or wholly outside;
                // the address is formed under the guard
                if (a.pl_y && yp < Hp) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int co = co0 + ct * 16 + r16;
                        if (co < a.Cout) {
                            float* row = a.pl_y + (int64_t)b * a.pl_y_bs + ((int64_t)co * Hp + yp) * Wp;
                            if (xp0 + 1 < Wp) *reinterpret_cast<float2*>(row + xp0) = make_float2(pm[ct][0], pm[ct][1]);
                            if (xp0 + 9 < Wp) *reinterpret_cast<float2*>(row + xp0 + 8) = make_float2(pm[ct][2], pm[ct][3]);
                        }
                    }
                }
            } else if (a.pl_y && yp < Hp && xp0 + 9 < Wp) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int co = co0 + ct * 16 + r16;
                    float* o = a.pl_y + (int64_t)b * a.pl_y_bs + ((int64_t)co * Hp + yp) * Wp + xp0;
                    if (co < a.Cout) {
                        *reinterpret_cast<float2*>(o) = make_float2(pm[ct][0], pm[ct][1]);
                        *reinterpret_cast<float2*>(o + 8) = make_float2(pm[ct][2], pm[ct][3]);
                    }
                }
            }
            if (a.pl_P) {
                const int c8 = r16 & 7, xs = xp0 + (c8 & 2 ? 8 : 0) + (c8 & 1);
                u32x4s* yP = reinterpret_cast<u32x4s*>(reinterpret_cast<unsigned*>(a.pl_P) + (int64_t)b * a.pl_P_bs);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const u32x4s slot = pre16_slot_transpose(pm[2 * p], pm[2 * p + 1], c8);
                    const int g8 = (co0 >> 3) + 2 * (2 * p + (c8 >> 2)) + (r16 >> 3);
                    if (yp < Hp && xs < Wp) yP[((int64_t)g8 * Hp + yp) * Wp + xs] = slot;
                }
            }
        }
        if constexpr (RD) {
            // RD, part 2: BatchNorm-backward reduce of the unit below (bn_relu_bwd_reduce_kernel's sums) from the tile in registers: dy = da
            // where that unit's output was positive, (sum dy, sum dy xhat) per channel.  Lane = channel, 16 pixel values: in-lane fp32
            // sums, the four lane groups by two shuffles, the eight waves through LDS in fp64 -> one record per tile and channel.  The
            // pass that read (da, z) -- 8 bytes per element -- becomes a 4-byte (2-byte: stored bf16) read of z here.
            __builtin_amdgcn_sched_barrier(0);
            float* sc = reinterpret_cast<float*>(lds + (buf ^ 1) * BUF);       // [8 waves][64 channels][s, sx]
            float vmax = 0.f;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int co = co0 + ct * 16 + r16, cc = min(co, a.Cout - 1);
                const float mean = rd_sv[cc], invstd = rd_sv[a.Cout + cc], scl = rd_sv[2 * a.Cout + cc], sh = rd_sv[3 * a.Cout + cc];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        const int yo = y0 + wn * NT + n, xo = (W16 ? 0 : x0 + 16 * ch) + 4 * lq;
                        if (co < a.Cout && yo < a.H && xo < a.W) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float da = acc[ct][n][ch][r], d = zr[ct][n][ch][r] - mean;
                                const float dy = fmaf(d, scl, sh) > 0.f ? da : 0.f;
                                s1 += dy;
                                s2 = fmaf(dy, d * invstd, s2);
                                vmax = fmaxf(vmax, fabsf(da));
                            }
                        }
                    }
                s1 += __shfl_xor(s1, 16, 64);
                s2 += __shfl_xor(s2, 16, 64);
                s1 += __shfl_xor(s1, 32, 64);
                s2 += __shfl_xor(s2, 32, 64);
                if (lq == 0) {
                    sc[(wn * 64 + ct * 16 + r16) * 2] = s1;
                    sc[(wn * 64 + ct * 16 + r16) * 2 + 1] = s2;
                }
            }
            if (a.rd_amax) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
                if (lane == 0 && vmax == vmax) atomicMax(a.rd_amax + ((blockIdx.x * 8 + wn) & (AMAX_SLOTS - 1)) * AMAX_STRIDE, __builtin_bit_cast(unsigned, vmax));
            }
            __syncthreads();
            if (tid < 64 && co0 + tid < a.Cout) {
                double t1 = 0.0, t2 = 0.0;
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    t1 += (double)sc[(w * 64 + tid) * 2];
                    t2 += (double)sc[(w * 64 + tid) * 2 + 1];
                }
                const int64_t blk = ((int64_t)b * a.tilesY + ty) * a.tilesX + tx;
                float* o = a.rd_rec + (blk * a.Cout + co0 + tid) * 4;
                o[0] = (float)t1;
                o[1] = (float)(t1 - (double)o[0]);
                o[2] = (float)t2;
                o[3] = (float)(t2 - (double)o[2]);
            }
            __syncthreads();
        }
    }
}

// The launch of a persistent tile-walking kernel: its dynamic LDS size once per device, then one 8-wave block per CU -- a multiple of the
// 8 XCDs (sp_tile_range), no more blocks than tiles rounded up to 8.  `once`: the kernel instance's own flag
template <class Args>
int sp_launch_persistent(void (*kern)(Args), PerDeviceOnce& once, int lds_bytes, int64_t tiles, int block, const char* name, const Args& a, hipStream_t st) {
    if (once.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    }
    const int64_t resident = (int64_t)device_cu_count();
    const int64_t blocks = std::min<int64_t>((tiles + 7) / 8 * 8, std::max<int64_t>(8, resident / 8 * 8));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(block), lds_bytes, st, a);
    return check_launch(name);
}

template <bool ST, int PM, bool W16, bool RD = false, bool ACT = false, bool HEAD = false, bool POOL = false, bool RAG = false, bool ANY = false>
int launch_split_pre(SpPreArgs a, hipStream_t st) {
    using C = SpPreCfg<W16>;
    const int LDS_BYTES = C::LDS_BYTES + (ST ? C::NW * 64 * 2 * 4 : 0) + (ACT || HEAD ? 2 * 3 * 64 * 4 : 0);
    a.tilesX = W16 ? 1 : cdiv(a.W, C::TW);
    a.tilesY = cdiv(a.H, C::ROWS);
    a.coTiles = cdiv(a.Cout, C::CO_T);
    if (W16 && ACT) {                                // tiles hold image pairs; an odd count: the last tile holds one image
        a.n_img = a.B;
        a.B = (a.B + 1) / 2;
    } else if (W16) {
        a.B /= 2;                                    // tiles hold image pairs
    }
    const int64_t tiles = (int64_t)a.B * a.tilesX * a.tilesY * a.coTiles;
    ONET_REQUIRE(tiles > 0 && tiles < (1ll << 31), "conv3x3_split_pre: tile count %lld out of range", (long long)tiles);
    // which launches take the 16x16x32 kernel (profiles/r05_mfma_shape_ab.md): plain bf16 operands (K = 32 channels: no packing) always; the
    // (hi | mid) forward WITH the statistics epilogue and the input gradients that carry the fused reduce (the lane layout's cheap
    // epilogues: -5 %); the plain (hi | mid) input gradient keeps the 32x32x16 kernel (equal speed), and so does the (hi | mid) 16-pixel
    // level (that instance of the new kernel exceeds the register budget).  The head epilogue exists on the 16x16x32 kernel alone.
    constexpr bool P16 = RD || PM == 2 || (ST && !W16) || HEAD;
    void (*kern)(SpPreArgs);
    static_assert(!ANY || P16, "launch_split_pre: the any-map instance exists on the 16x16x32 kernel alone");
    if constexpr (P16) kern = conv3x3_pre16_kernel<ST, PM, W16, RD, ACT, HEAD, POOL, RAG, ANY>;      // (constexpr: the instances not dispatched are not built)
    else kern = conv3x3_split_pre_kernel<ST, PM, W16, ACT, POOL, RAG>;
    static PerDeviceOnce attr_once;
    return sp_launch_persistent(kern, attr_once, LDS_BYTES, tiles, C::NW * 64,
                                HEAD   ? (PM == 2 ? "conv3x3_pre16_head_kernel" : "conv3x3_split_pre_head_kernel")
                                : POOL ? (PM == 2 ? "conv3x3_pre16_act_pool_kernel" : "conv3x3_split_pre_act_pool_kernel")
                                : ACT  ? (W16 ? (PM == 2 ? "conv3x3_pre16_act_pairs_kernel" : "conv3x3_split_pre_act_pairs_kernel")
                                              : PM == 2 ? "conv3x3_pre16_act_kernel" : "conv3x3_split_pre_act_kernel")
                                      : "conv3x3_split_pre_kernel", a, st);
}

int split_nparts(int B, int H, int W) {
    if (B <= 0 || W < 32 || (W % SpCfg::TW) || (H % SpCfg::ROWS)) return 0;
    const int64_t n = (int64_t)B * (H / SpCfg::ROWS) * (W / SpCfg::TW);
    return n < (1 << 30) ? (int)n : 0;
}

template <bool ST, bool NORM, bool F16>
int launch_split(SpArgs a, hipStream_t st) {
    using C = SpCfg;
    const int LDS_BYTES = C::LDS_BYTES + (ST ? C::NW * 64 * 2 * 4 : 0) + (NORM ? 2 * 2 * 8 * 4 * 4 : 0);
    a.tilesX = cdiv(a.W, C::TW);
    a.tilesY = cdiv(a.H, C::ROWS);
    a.coTiles = cdiv(a.Cout, C::CO_T);
    const int64_t tiles = (int64_t)a.B * a.tilesX * a.tilesY * a.coTiles;
    ONET_REQUIRE(tiles > 0 && tiles < (1ll << 31), "conv3x3_split: tile count %lld out of range", (long long)tiles);
    static PerDeviceOnce attr_once;
    return sp_launch_persistent(conv3x3_split_kernel<ST, NORM, F16>, attr_once, LDS_BYTES, tiles, 512, "conv3x3_split_kernel", a, st);
}

int split_fwd(const float* x, int64_t x_bs, const void* wq, float* z, int64_t z_bs, int B, int Cin, int Cout, int H, int W,
              void* stream, float* stats, int wq_f16, const float* nsave = nullptr, int n_groups = 0, const unsigned* x_amax = nullptr,
              int x_always = 0) {
    ONET_REQUIRE(x && wq && z, "conv3x3_split_fwd: null pointer");
    ONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 16, "conv3x3_split_fwd: bad shape (maps wider than 16 pixels)");
    ONET_REQUIRE((Cin % 16) == 0, "conv3x3_split_fwd: Cin must be a multiple of 16 (use onet_conv_fwd)");
    ONET_REQUIRE((W & 3) == 0 && (x_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                 "conv3x3_split_fwd: W %% 4 == 0 and 16-byte aligned image rows required (use onet_conv3x3_winograd4_fwd)");
    ONET_REQUIRE(x_bs >= (int64_t)Cin * H * W && z_bs >= (int64_t)Cout * H * W, "conv3x3_split_fwd: batch stride too small");
    ONET_REQUIRE((int64_t)(Cin + 32) * H * W * 4 < (1ll << 31) && (int64_t)(Cin + 32) * 2 * 9 * Cout * 2 < (1ll << 31),
                 "conv3x3_split_fwd: operand exceeds the 2 GiB buffer-resource range");
    SpArgs a{x, x_bs, (const __bf16*)wq, z, z_bs, B, Cin, Cout, H, W, 0, 0, 0, stats, nsave, 1, x_amax, x_always};
    ONET_REQUIRE(!x_amax || wq_f16, "conv3x3_split: magnitude slots go with the fp16 pack");
    if (stats) ONET_REQUIRE(split_nparts(B, H, W) > 0, "conv3x3_split_fwd_stats: the map must be made of full 16 x 32 tiles");
    if (nsave) {
        ONET_REQUIRE(n_groups > 0 && B % n_groups == 0, "conv3x3_split_fwd_norm: the batch must hold n_groups equal statistics groups");
        a.nimg = B / n_groups;
        if (wq_f16) return stats ? launch_split<true, true, true>(a, as_stream(stream)) : launch_split<false, true, true>(a, as_stream(stream));
        return stats ? launch_split<true, true, false>(a, as_stream(stream)) : launch_split<false, true, false>(a, as_stream(stream));
    }
    if (wq_f16) return stats ? launch_split<true, false, true>(a, as_stream(stream)) : launch_split<false, false, true>(a, as_stream(stream));
    return stats ? launch_split<true, false, false>(a, as_stream(stream)) : launch_split<false, false, false>(a, as_stream(stream));
}


// ------------------------------------------------------------------ weight gradient, split operands
//   dW[co][ci][ky][kx] = sum_{b,y,x} dz[b][co][y][x] * X[b][ci][y+ky-1][x+kx-1]:  M = co, N = ci, K = pixels, one accumulator per
//   tap, v_mfma_f32_32x32x16_bf16 with the 8 K-values of a lane = 8 consecutive pixels of one channel row.  The row-streaming
//   structure (first used by round 2's bf16 weight gradient, DESIGN_HISTORY.md 4.2d): a unit is ONE image row of a 64-pixel strip -- dz [64 co][64 px],
//   x rows y-1, y, y+1 [64 ci][66 px] in a 4-slot ring, a block walks down its strip and loads one new row of each operand per
//   unit as whole 128-byte lines -- with both operands split on the way into LDS (hi | mid parts of dz and of x) and three MFMAs
//   per (16-pixel segment, tap): dz_mid x_hi + dz_hi x_mid + dz_hi x_hi.  110 KB of LDS: one block per CU, of EIGHT waves -- two
//   groups of four that split a unit's four segments between them and keep their own accumulators (a split over K inside the
//   block: 4 waves at one per SIMD had nothing to cover the barrier, the commit and the fragment reads, 0.33 of the bf16 peak);
//   54 MFMAs per wave and unit.  Split-K over (image, strip, row) units, raw slabs [split][tap][co][ci] reduced deterministically by
//   wgrad_reduce_kernel (conv_mfma.hip).  Requires W >= 64 with W % 4 == 0, or W = 32 / 16 (below).
struct SwArgs {
    const float* x;
    int64_t x_bs;
    const float* dz;
    int64_t dz_bs;
    float* slab;
    int B, Cin, Cout, H, W, ciTiles, coTiles, splitK, tilesX;
    const float* nsave;   // NORM: x is the pre-activation of the unit below, normalised on load (see conv3x3_split_kernel): its
    int nimg;             //       coefficients [groups <= 2][4][Cin], statistics groups of nimg consecutive images
    const unsigned* x_amax;    // F16: magnitude slots of x (overflow guard only; NULL: unscaled) and of dz (always scaled: amax
    const unsigned* dz_amax;   //      lands in [2^13, 2^14)); the slab store undoes both scales
};

// Maps narrower than a strip (G = 64 / W = 2 or 4: the 32- and 16-pixel levels): a unit is row y of G IMAGES side by side -- the dz
// row is their 64 pixels back to back, the x row keeps each image's own halo (sub-row pitch SR_P dwords: W / 2 data dwords + the
// right-halo dword, rounded to 16 bytes), so a horizontal shift never reads a neighbouring image's pixel.  Everything else -- the
// ring over rows, the two pixel groups, the commit inside the MFMA block -- is the 64-pixel strip's.
constexpr int SR_SDZ = 36;                                  // dword stride per co
template <int G> struct SwCfg {
    static constexpr int SPG = 8 / G;                       // 8-pixel segments per sub-row
    static constexpr int P = G == 1 ? 36 : (G == 2 ? 20 : 12);
    static constexpr int SLOT = G * P;                      // 36 / 40 / 48 dwords per ring slot
    static constexpr int SX = 4 * SLOT + 4;                 // per ci: 148 / 164 / 196 = 4 x odd
    static constexpr int X_PART = 64 * SX;
    static constexpr int GOFF = G == 1 ? 16 : (G == 2 ? 20 : 24);   // fragment offset of pixel group 1 / of segment 1
    static constexpr int SOFF = G == 4 ? 12 : 8;
};

// COT = output channels per block.  64: the 8 waves are two K-groups x (2 x 2) quadrants, group g takes the 16-pixel segments 2g,
// 2g + 1 of a unit and writes its own slab (54 MFMAs per wave between barriers).  128 (Cout % 128 == 0, G < 4: the LDS holds
// it): 4 x 2 quadrants, every wave takes all four segments -- 108 MFMAs per wave between barriers, the x rows staged once per
// 128 output channels, one slab per block.
// F16: fp16 parts (22 significant bits per operand instead of bf16's 16) of 2^kx x and 2^kd dz -- see amax_scale
template <int G, int COT, bool NORM, bool F16>
__global__ __launch_bounds__(512, 2) void conv3x3_split_wgrad_kernel(SwArgs a) {
    using C = SwCfg<G>;
    constexpr int SR_SX = C::SX, SR_SLOT = C::SLOT, SR_X_PART = C::X_PART;
    constexpr int SR_DZ_PART = COT * SR_SDZ;
    constexpr int NSEG = COT == 64 ? 2 : 4;                  // 16-pixel segments per wave and unit
    constexpr int DZI = COT / 64;                            // dz staging items (8 pixels of one channel) per thread
    __shared__ __attribute__((aligned(16))) unsigned dz_lds[2 * 2 * SR_DZ_PART];     // [buf][part][COT co][SR_SDZ]
    __shared__ __attribute__((aligned(16))) unsigned x_lds[2 * SR_X_PART];           // [part][64 ci][SR_SX]

    int bid = xcd_block_id();
    const int tiles = a.ciTiles * a.coTiles;
    const int ks = bid / tiles, tile = bid % tiles;
    const int ci0 = (tile % a.ciTiles) * 64, co0 = (tile / a.ciTiles) * COT;
    const int nunits = (a.B / G) * a.tilesX * a.H;             // unit = (image [group of G], 64-pixel strip, row), rows fastest
    const int per = (nunits + a.splitK - 1) / a.splitK;
    const int u0 = ks * per, u1 = min(u0 + per, nunits);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int grp = COT == 64 ? wid >> 2 : 0, wm = COT == 64 ? (wid >> 1) & 1 : wid >> 1, wn = wid & 1;
    const int l31 = lane & 31, kh = lane >> 5;
    const int HW = a.H * a.W;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float x_inv = 1.f, dz_inv = 1.f;
    const float x_scale = F16 ? amax_scale(amax_read(a.x_amax), false, x_inv) : 1.f;
    const float dz_scale = F16 ? amax_scale(amax_read(a.dz_amax), true, dz_inv) : 1.f;

    // staging roles: thread = (channel = tid / 8, 8-pixel segment = tid % 8) of the dz row and of the x row
    const int st_c = tid >> 3, st_s = tid & 7;
    const int st_sub = st_s / C::SPG, st_w = st_s % C::SPG;     // image of the group, 8-pixel segment of its row
    u32x4s dzv[2 * DZI], xq[2];
    float xh[2];
    // NORM: BatchNorm coefficients of this thread's x channel for the (at most two) statistics groups; the group and the
    // validity of the row whose loads are in flight
    float n_mean[2] = {0.f, 0.f}, n_sc[2] = {0.f, 0.f}, n_sh[2] = {0.f, 0.f};
    bool pend_v[4] = {false, false, false, false}, pend_g1 = false;      // left halo | pixels 0-3 | pixels 4-7 | right halo
    if constexpr (NORM) {
        const int ch = min(ci0 + st_c, a.Cin - 1), last = a.B / a.nimg - 1;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float* sv = a.nsave + (int64_t)min(g, last) * 4 * a.Cin + ch;
            n_mean[g] = sv[0];
            n_sc[g] = sv[2 * a.Cin];
            n_sh[g] = sv[3 * a.Cin];
        }
    }
    // loads of one dz row and / or one x row of strip (b, x0): row < 0 or >= H -> zeros.  G == 1: one buffer resource per image
    // (a 256 x 256 level's batch exceeds the 2 GiB range); G > 1: the lanes of a wave address different images, so the resource
    // spans the whole (small) tensor and the image offset goes into the lane's byte offset (range checked by the host)
    auto issue_dz = [&](int b, int x0, int y, int p0 = 0, int p1 = 64) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t dr = G == 1 ? s_rsrc(a.dz + (int64_t)b * a.dz_bs, (int64_t)a.Cout * HW * 4)
                                                 : s_rsrc(a.dz, ((int64_t)(a.B - 1) * a.dz_bs + (int64_t)a.Cout * HW) * 4);
        const int xs = x0 + 8 * st_w;
#pragma unroll
        for (int i = 0; i < DZI; ++i) {
            const int co = co0 + st_c + 64 * i;
            const bool ok = y >= 0 && y < a.H && co < a.Cout;
            const unsigned base = (unsigned)((co * HW + y * a.W + xs) * 4) + (G == 1 ? 0u : (unsigned)((int64_t)(b * G + st_sub) * a.dz_bs * 4));
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (2 * i + k >= p0 && 2 * i + k < p1)
                    dzv[2 * i + k] = __builtin_amdgcn_raw_buffer_load_b128(dr, (ok && xs + 4 * k < a.W) ? base + 16 * k : OOB_S, 0, 0);
        }
    };
    auto issue_x = [&](int b, int x0, int y, int p0 = 0, int p1 = 64) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t xr = G == 1 ? s_rsrc(a.x + (int64_t)b * a.x_bs, (int64_t)a.Cin * HW * 4)
                                                 : s_rsrc(a.x, ((int64_t)(a.B - 1) * a.x_bs + (int64_t)a.Cin * HW) * 4);
        const int xs = x0 + 8 * st_w;
        const bool ok = y >= 0 && y < a.H && ci0 + st_c < a.Cin;
        const unsigned base = (unsigned)(((ci0 + st_c) * HW + y * a.W + xs) * 4) + (G == 1 ? 0u : (unsigned)((int64_t)(b * G + st_sub) * a.x_bs * 4));
        if (NORM && p0 == 0) {
            pend_v[0] = ok && xs > 0 && xs - 1 < a.W;
            pend_v[1] = ok && xs < a.W;
            pend_v[2] = ok && xs + 4 < a.W;
            pend_v[3] = ok && st_w == C::SPG - 1 && xs + 8 < a.W;
            pend_g1 = (G == 1 ? b : b * G + st_sub) >= a.nimg;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k >= p0 && k < p1) xq[k] = __builtin_amdgcn_raw_buffer_load_b128(xr, (ok && xs + 4 * k < a.W) ? base + 16 * k : OOB_S, 0, 0);
        if (2 >= p0 && 2 < p1)
            xh[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (ok && xs > 0 && xs - 1 < a.W) ? base - 4 : OOB_S, 0, 0));
        if (3 >= p0 && 3 < p1)
            xh[1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (ok && st_w == C::SPG - 1 && xs + 8 < a.W) ? base + 32 : OOB_S, 0, 0));
    };
    auto commit_dz = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < DZI; ++i) {
            unsigned* d = dz_lds + buf * 2 * SR_DZ_PART + (st_c + 64 * i) * SR_SDZ + st_s * 4;
            // (the whole vector is re-typed, then indexed: element-wise bit casts of the loaded vector's lanes came out as four
            // copies of lane 0 with hipcc 7.2 -- found with delta-function inputs)
            const f32x4s lo = __builtin_bit_cast(f32x4s, dzv[2 * i]), hv = __builtin_bit_cast(f32x4s, dzv[2 * i + 1]);
            const float f[8] = {lo[0], lo[1], lo[2], lo[3], hv[0], hv[1], hv[2], hv[3]};
            u32x4s hi, mid;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                unsigned hh, mm;
                if constexpr (F16) split2h_s(f[2 * c], f[2 * c + 1], dz_scale, hh, mm);
                else split2(f[2 * c], f[2 * c + 1], hh, mm);
                hi[c] = hh;
                mid[c] = mm;
            }
            *reinterpret_cast<u32x4s*>(d) = hi;
            *reinterpret_cast<u32x4s*>(d + SR_DZ_PART) = mid;
        }
    };
    // row element e = column x0 - 1 + e; dword p = (e[2p], e[2p+1]) = (f[2p-1], f[2p]) of the interior row f: an 8-pixel segment's
    // four dwords start with (pixel left of the segment, its first pixel); its last pixel opens the next segment's first dword
    // (loaded there as that segment's left neighbour); the strip's last dword (f[63], right halo) is segment 7's
    auto commit_x = [&](int slot) __attribute__((always_inline)) {
        unsigned* row = x_lds + st_c * SR_SX + slot * SR_SLOT + st_sub * C::P + st_w * 4;
        const f32x4s f0 = __builtin_bit_cast(f32x4s, xq[0]), f1 = __builtin_bit_cast(f32x4s, xq[1]);
        float e[10] = {xh[0], f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3], xh[1]};
        if constexpr (NORM) {
            // the activation bn_relu_apply_kernel would have written, element for element; what lies outside the image (rows
            // above / below, the strip's halo columns at the image border) is the convolution's zero padding and stays zero
            const float mean = pend_g1 ? n_mean[1] : n_mean[0], sc = pend_g1 ? n_sc[1] : n_sc[0], sh = pend_g1 ? n_sh[1] : n_sh[0];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const float v = fmaxf(fmaf(e[k] - mean, sc, sh), 0.f);
                e[k] = pend_v[k == 0 ? 0 : (k <= 4 ? 1 : (k <= 8 ? 2 : 3))] ? v : 0.f;
            }
        }
        unsigned hi[5], mid[5];
#pragma unroll
        for (int p2 = 0; p2 < 5; ++p2) {
            if constexpr (F16) split2h_s(e[2 * p2], e[2 * p2 + 1], x_scale, hi[p2], mid[p2]);
            else split2(e[2 * p2], e[2 * p2 + 1], hi[p2], mid[p2]);
        }
        *reinterpret_cast<u32x4s*>(row) = u32x4s{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<u32x4s*>(row + SR_X_PART) = u32x4s{mid[0], mid[1], mid[2], mid[3]};
        if (st_w == C::SPG - 1) {
            row[4] = hi[4];
            row[SR_X_PART + 4] = mid[4];
        }
    };

    const unsigned* a_ptr = dz_lds + (wm * 32 + l31) * SR_SDZ + kh * 4 + grp * 16;
    const unsigned* b_ptr = x_lds + (wn * 32 + l31) * SR_SX + kh * 4 + grp * C::GOFF;
    // x-row dword offset of segment s of a wave: pixel groups 2 s, 2 s + 1 -> sub-row (2 s) / SPG, position (2 s) % SPG
    auto seg_off = [](int sg) { return G == 1 ? sg * 8 : (G == 2 ? (sg >> 1) * 20 + (sg & 1) * 8 : sg * 12); };

    int u = u0;
    while (u < u1) {
        // a run of rows inside one strip: y = yb .. ye - 1
        const int yb = u % a.H, sb = u / a.H;
        const int tx = sb % a.tilesX, b = sb / a.tilesX;
        const int x0 = G == 1 ? tx * 64 : 0;
        const int ye = min(a.H, yb + (u1 - u));
        // run prologue: rows yb - 1 and yb of x into the ring (synchronously), then the dz row and the next x row of the first unit
        __syncthreads();                              // every wave is done with the previous run's ring and dz buffers
        issue_x(b, x0, yb - 1);
        commit_x((yb - 1) & 3);
        issue_x(b, x0, yb);
        commit_x(yb & 3);
        issue_dz(b, x0, yb);
        issue_x(b, x0, yb + 1);
        commit_dz(yb & 1);
        commit_x((yb + 1) & 3);
        __syncthreads();
        if (yb + 1 < ye) {
            issue_dz(b, x0, yb + 1);
            issue_x(b, x0, yb + 2);
        }
        __builtin_amdgcn_sched_barrier(0);
        for (int y = yb; y < ye; ++y) {
            // unit y: MFMAs on dz buffer y & 1 and ring rows y - 1 .. y + 1.  Staging rides inside the MFMA block: the rows of unit
            // y + 1 (in registers since the previous unit) are split and committed after the first MFMA group -- into the other dz
            // buffer and the ring slot of row y - 2, both last read in unit y - 1 -- and the loads of unit y + 2's rows then go
            // out ONE PER MFMA GROUP.  (Issued as a burst behind the barrier, by all eight waves at once, they held every wave's
            // issue port while the matrix pipe idled: a timing build without them ran 16 % faster, one without the barrier 4 %.)
            const int buf = y & 1;
            const bool more = y + 1 < ye, more2 = y + 2 < ye;
            const unsigned* ab = a_ptr + buf * 2 * SR_DZ_PART;
            u32x4s ah, am;
            // MFMA groups of the unit (of 6 with 64-channel tiles, 12 with 128) before the next unit's rows are committed
            constexpr int CAT = COT == 64 ? 2 : 5;
            // Segments run LAST TO FIRST: a lane's 8-pixel fragment is one aligned ds_read_b128 (4 dwords); the fifth dword its
            // shifted copies need is the first dword of the NEXT 8-pixel group -- for the kh = 0 half that of its kh = 1 partner in
            // the same read, for the kh = 1 half that of the kh = 0 lane of the segment read one group earlier: both arrive by
            // v_permlane32_swap instead of a ds_read_b32, which on a row stride that is a multiple of 4 dwords is a 4-way bank
            // conflict (20 l mod 32 repeats every 8 lanes; SQ_LDS_BANK_CONFLICT was 63 % of the kernel's LDS cycles, the LDS 70 %
            // busy).  Only where the next group is another image's or the strip's halo does the dword still come from LDS.
            unsigned lo_prev[3][2] = {};
#pragma unroll
            for (int gk = 0; gk < 3 * NSEG; ++gk) {
                const int sg = NSEG - 1 - gk / 3, ky = gk % 3;
                const bool from_prev = (sg + 1 < NSEG) && (G == 1 || (G == 2 && (sg & 1) == 0));
                if (gk == CAT && more) {
                    commit_dz(buf ^ 1);
                    commit_x((y + 2) & 3);
                }
                if (more2) {
                    // pieces: 2 DZI dz loads, then the four x loads; groups CAT + 1 ... (two or more pieces each where
                    // they do not fit one per group)
                    constexpr int NP = 2 * DZI + 4, NG = 3 * NSEG - CAT - 1, PER = (NP + NG - 1) / NG;
                    const int g0 = gk - CAT - 1;
                    if (g0 >= 0) {
#pragma unroll
                        for (int q = 0; q < PER; ++q) {
                            const int pc = g0 * PER + q;
                            if (pc < 2 * DZI) issue_dz(b, x0, y + 2, pc, pc + 1);
                            else if (pc < NP) issue_x(b, x0, y + 3, pc - 2 * DZI, pc - 2 * DZI + 1);
                        }
                    }
                }
                if (ky == 0) {
                    ah = *reinterpret_cast<const u32x4s*>(ab + sg * 8);
                    am = *reinterpret_cast<const u32x4s*>(ab + SR_DZ_PART + sg * 8);
                }
                const unsigned* br = b_ptr + ((y - 1 + ky) & 3) * SR_SLOT + seg_off(sg);
                u32x4s sh[2][3];                  // [part][horizontal shift]
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    const u32x4s q = *reinterpret_cast<const u32x4s*>(br + pt * SR_X_PART);
                    unsigned d4;
                    if (G == 4) {
                        d4 = br[pt * SR_X_PART + 4];
                    } else {
                        const auto sw = __builtin_amdgcn_permlane32_swap(q[0], q[0], false, false);   // [0]: the kh = 0 value in
                        const unsigned nxt = from_prev ? lo_prev[ky][pt] : br[pt * SR_X_PART + 4];       // both halves, [1]: kh = 1's
                        d4 = kh ? nxt : sw[1];
                        lo_prev[ky][pt] = sw[0];
                    }
                    sh[pt][0] = q;
                    sh[pt][1] = u32x4s{__builtin_amdgcn_alignbit(q[1], q[0], 16), __builtin_amdgcn_alignbit(q[2], q[1], 16),
                                       __builtin_amdgcn_alignbit(q[3], q[2], 16), __builtin_amdgcn_alignbit(d4, q[3], 16)};
                    sh[pt][2] = u32x4s{q[1], q[2], q[3], d4};
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if constexpr (F16) {
                        const f16x8 a_h = __builtin_bit_cast(f16x8, ah), a_m = __builtin_bit_cast(f16x8, am);
                        const f16x8 bh = __builtin_bit_cast(f16x8, sh[0][j]), bm = __builtin_bit_cast(f16x8, sh[1][j]);
                        acc[ky * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_m, bh, acc[ky * 3 + j], 0, 0, 0);
                        acc[ky * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h, bm, acc[ky * 3 + j], 0, 0, 0);
                        acc[ky * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h, bh, acc[ky * 3 + j], 0, 0, 0);
                    } else {
                        const bf16x8 a_h = __builtin_bit_cast(bf16x8, ah), a_m = __builtin_bit_cast(bf16x8, am);
                        const bf16x8 bh = __builtin_bit_cast(bf16x8, sh[0][j]), bm = __builtin_bit_cast(bf16x8, sh[1][j]);
                        acc[ky * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_m, bh, acc[ky * 3 + j], 0, 0, 0);
                        acc[ky * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, bm, acc[ky * 3 + j], 0, 0, 0);
                        acc[ky * 3 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, bh, acc[ky * 3 + j], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        }
        u += ye - yb;
    }

    const int64_t n = (int64_t)a.Cout * a.Cin;
    const int ci = ci0 + wn * 32 + l31;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* o = a.slab + ((int64_t)(COT == 64 ? ks * 2 + grp : ks) * 9 + t) * n;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < a.Cout && ci < a.Cin) o[(int64_t)co * a.Cin + ci] = F16 ? acc[t][r] * (x_inv * dz_inv) : acc[t][r];
        }
    }
}

// ------------------------------------------------------------------ weight gradient from PRE-SPLIT operands (round 4)
// Both operands arrive in the slot layout [B][C/8][H][part][W][8] (16 bytes = 8 channels of one pixel), i.e. with the reduction
// index (pixels) running ACROSS slots.  The MFMA wants 8 consecutive pixels of one channel per lane, so the fragments are read
// with the gfx950 transposing LDS read ds_read_b64_tr_b16 (a 16-lane group fetches 4 pixel rows x 16 channels and every lane
// receives ITS channel's four pixels): no in-kernel split, no transposition VALU, and a tap's horizontal shift is a pixel-row
// offset of the read address (the round-3 kernel rebuilt shifted fragments with v_alignbit + v_permlane32_swap).  Staging is a
// lane-linear LDS-DMA copy as in conv3x3_split_pre_kernel.  Unit, ring over rows, split-K and slabs as conv3x3_split_wgrad_kernel.
//   x ring : [4 row slots][part][8 channel groups][PXP = 68 pixel slots]   (G = 1: x0-1 .. x0+64 + 2 pad; G = 2: two images' 34)
//   dz     : [2 buffers] [part][COT / 8 groups]  [PXP = 68]                (64 pixels + 4 pad)
// A channel group's plane of 68 slots = 272 dwords = 16 banks (mod 64): the 4 pixel rows x (2 groups x 2 half-slots) a 32-lane
// half reads fall on 64 different banks -- conflict-free without a swizzle.
typedef short s16x4w __attribute__((ext_vector_type(4)));
struct SwPreArgs {
    const void* xs;
    int64_t xs_bs;        // batch strides in 4-byte units
    const void* dzs;
    int64_t dzs_bs;
    float* slab;
    int B, Cin, Cout, H, W, ciTiles, coTiles, splitK, tilesX;
    const unsigned* x_slots;    // magnitude slots the producers scaled the operands by (NULL: unscaled); x: guard rule, dz: always
    const unsigned* dz_slots;
    const unsigned* x_slots2;   // concat buffer: input channels >= split_ch (a multiple of 64) were scaled by these (NULL: unscaled)
    int split_ch;
};
constexpr int SWP_PXP = 68;          // G = 4 (16-pixel maps: four images of 18 slots each): 76 (304 dwords = 48 banks mod 64: conflict-free too)

__device__ __forceinline__ u32x4s swp_frag(unsigned addr) {      // 8 consecutive pixels (K) of this lane's channel: two transposed reads
    const s16x4w lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4w*)(uintptr_t)addr);
    const s16x4w hv = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4w*)(uintptr_t)(addr + 64));
    const unsigned long long a = __builtin_bit_cast(unsigned long long, lo), b = __builtin_bit_cast(unsigned long long, hv);
    return u32x4s{(unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)};
}

// The MFMA shape is v_mfma_f32_16x16x32 (profiles/r05_mfma_shape_ab.md: the shape the chip clocks higher on).  K = pixels here, so
// K = 32 is natural -- one instruction takes 32 consecutive pixels of a unit's row, no K-packing.  A wave's 32 x 32 channel tile per
// tap is four 16 x 16 accumulators; M = input channels (A = x fragment), N = output channels (B = dz fragment), so a lane owns four
// CONSECUTIVE input channels of one output channel and the slab leaves as float4 stores.  Lane group lg = lane / 16 takes pixels
// 8 lg .. 8 lg + 7 of the step (G = 4, four 16-pixel images per unit: lane groups 0-1 / 2-3 sit in two different images' sub-rows).
// PM: 0 bf16 (hi | mid), 1 fp16 (hi | mid) -- three MFMAs per term; 2: PLAIN bf16 operands, one part (BASELINE configs[2]), one MFMA
template <int G, int COT, int PM>
__global__ __launch_bounds__(512, 2) void conv3x3_wgrad_pre16_kernel(SwPreArgs a) {
    constexpr bool F16 = PM == 1;
    constexpr int NP = PM == 2 ? 1 : 2;                        // parts per operand
    constexpr int PXP = G == 4 ? 76 : SWP_PXP;
    constexpr int XS = 8, DS = COT / 8;                        // channel groups per image
    // (row images padded to whole 64-slot DMA pieces: the lanes of a piece beyond the image write zeros, which must not land in the
    // next ring slot / buffer)
    constexpr int X_PART = XS * PXP, X_ROW = (NP * X_PART + 63) / 64 * 64;      // slots
    constexpr int DZ_PART = DS * PXP, DZ_BUF = (NP * DZ_PART + 63) / 64 * 64;
    constexpr int NXI = (X_ROW + 511) / 512, NDI = (DZ_BUF + 511) / 512;      // DMA rounds per wave (64 slots each, 8 waves)
    constexpr int NKS = COT == 64 ? 1 : 2;                     // k-steps (32 pixels) per wave and unit
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_w[];
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_w;
    const unsigned x_base = lds0, dz_base = lds0 + 4 * X_ROW * 16;

    int bid = xcd_block_id();
    const int tiles = a.ciTiles * a.coTiles;
    const int ks = bid / tiles, tile = bid % tiles;
    const int ci0 = (tile % a.ciTiles) * 64, co0 = (tile / a.ciTiles) * COT;
    const int nunits = (a.B / G) * a.tilesX * a.H;
    const int per = (nunits + a.splitK - 1) / a.splitK;
    const int u0 = ks * per, u1 = min(u0 + per, nunits);

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = COT == 64 ? wid >> 2 : 0, wm = COT == 64 ? (wid >> 1) & 1 : wid >> 1, wn = wid & 1;
    const int r16 = lane & 15, lg = lane >> 4;
    const int HW = a.H * a.W;

    f32x4s acc[9][2][2];                                        // [tap][input-channel half (M)][output-channel half (N)]
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i >> 1][i & 1] = f32x4s{0.f, 0.f, 0.f, 0.f};

    // transposed-read lane bases (bytes): lane = 16 lg + 4 q + p supplies pixel row q (of the group's 8 pixels), channels 4 p .. 4 p + 3
    // of the 16-channel half; the wave's second half sits two channel groups (2 PXP slots) further
    const int tq = (lane >> 2) & 3, tp = lane & 3;
    const int xg = G == 4 ? (lg >> 1) * 18 + 8 * (lg & 1) : 8 * lg;              // x pixel slot of the lane group inside a 32-pixel step
    const unsigned a_lane = (unsigned)((((wm * 4 + (tp >> 1)) * PXP + 8 * lg + tq) * 16) + (tp & 1) * 8);       // dz
    const unsigned b_lane = (unsigned)((((wn * 4 + (tp >> 1)) * PXP + xg + tq) * 16) + (tp & 1) * 8);           // x
    constexpr unsigned HALF = 2 * PXP * 16;

    // ---- staging: slot position i = (wid + 8 k) * 64 + lane of a row image [part][group][PXP]
    i32x4s xr, dr;
    unsigned x_off[NXI], d_off[NDI];
    auto setup_strip = [&](int b, int x0) __attribute__((always_inline)) {
        if (G == 1) {
            xr = sp_rsrc4(reinterpret_cast<const unsigned*>(a.xs) + (int64_t)b * a.xs_bs, (int64_t)a.Cin * HW * 2 * NP);
            dr = sp_rsrc4(reinterpret_cast<const unsigned*>(a.dzs) + (int64_t)b * a.dzs_bs, (int64_t)a.Cout * HW * 2 * NP);
        } else {
            xr = sp_rsrc4(a.xs, (int64_t)(a.B - 1) * a.xs_bs * 4 + (int64_t)a.Cin * HW * 2 * NP);
            dr = sp_rsrc4(a.dzs, (int64_t)(a.B - 1) * a.dzs_bs * 4 + (int64_t)a.Cout * HW * 2 * NP);
        }
#pragma unroll
        for (int k = 0; k < NXI; ++k) {
            const int i = (wid + 8 * k) * 64 + lane;
            const int part = i / X_PART, s = (i % X_PART) / PXP, pi = i % PXP;
            const int img = G == 1 ? 0 : pi / (a.W + 2), xx = G == 1 ? x0 - 1 + pi : pi % (a.W + 2) - 1;
            const bool ok = i < NP * X_PART && pi < (G == 1 ? 66 : G * (a.W + 2)) && xx >= 0 && xx < a.W && ci0 + 8 * s < a.Cin;
            const int64_t img_off = G == 1 ? 0 : (int64_t)(b * G + img) * a.xs_bs * 4;
            x_off[k] = ok ? (unsigned)(img_off + ((int64_t)((ci0 / 8 + s) * a.H) * NP + part) * a.W * 16 + xx * 16) : OOB_S;
        }
#pragma unroll
        for (int k = 0; k < NDI; ++k) {
            const int i = (wid + 8 * k) * 64 + lane;
            const int part = i / DZ_PART, s = (i % DZ_PART) / PXP, pi = i % PXP;
            const int img = G == 1 ? 0 : pi / a.W, xx = G == 1 ? x0 + pi : pi % a.W;
            const bool ok = i < NP * DZ_PART && pi < 64 && xx < a.W && co0 + 8 * s < a.Cout;
            const int64_t img_off = G == 1 ? 0 : (int64_t)(b * G + img) * a.dzs_bs * 4;
            d_off[k] = ok ? (unsigned)(img_off + ((int64_t)((co0 / 8 + s) * a.H) * NP + part) * a.W * 16 + xx * 16) : OOB_S;
        }
    };
    // row y of the strip into ring slot / dz buffer; rows outside the image are zeros (every lane out of range)
    auto dma_x = [&](int y, int k) __attribute__((always_inline)) {
        if ((wid + 8 * k) * 64 < X_ROW) {
            const bool ok = y >= 0 && y < a.H;
            sp_dma16(xr, x_base + (unsigned)(((y & 3) * X_ROW + (wid + 8 * k) * 64) * 16), ok ? x_off[k] : OOB_S, ok ? (unsigned)(y * NP * a.W * 16) : 0u);
        }
    };
    auto dma_dz = [&](int y, int k) __attribute__((always_inline)) {
        if ((wid + 8 * k) * 64 < DZ_BUF) {
            const bool ok = y >= 0 && y < a.H;
            sp_dma16(dr, dz_base + (unsigned)(((y & 1) * DZ_BUF + (wid + 8 * k) * 64) * 16), ok ? d_off[k] : OOB_S, ok ? (unsigned)(y * NP * a.W * 16) : 0u);
        }
    };

    int u = u0;
    while (u < u1) {
        const int yb = u % a.H, sb = u / a.H;
        const int tx = sb % a.tilesX, b = sb / a.tilesX;
        const int x0 = G == 1 ? tx * 64 : 0;
        const int ye = min(a.H, yb + (u1 - u));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                              // every wave is done with the previous run's ring and dz buffers
        setup_strip(b, x0);
#pragma unroll
        for (int k = 0; k < NXI; ++k) {
            dma_x(yb - 1, k);
            dma_x(yb, k);
            dma_x(yb + 1, k);
        }
#pragma unroll
        for (int k = 0; k < NDI; ++k) dma_dz(yb, k);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int y = yb; y < ye; ++y) {
            // unit y: MFMAs on dz buffer y & 1 and ring rows y - 1 .. y + 1; the rows of unit y + 1 (dz row y + 1, x row y + 2) go
            // by DMA into the other dz buffer and the ring slot of row y - 2 (both last read in unit y - 1), spread over the k-steps
            const bool more = y + 1 < ye;
            const unsigned ab = dz_base + (unsigned)((y & 1) * DZ_BUF * 16) + a_lane;
            unsigned bb[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) bb[ky] = x_base + (unsigned)((((y - 1 + ky) & 3) * X_ROW) * 16) + b_lane;
#pragma unroll
            for (int kk = 0; kk < NKS; ++kk) {
                const int kst = COT == 64 ? grp : kk;                          // 32-pixel k-step of the unit
                const int dpx = 32 * kst;                                      // dz pixel slot
                const int xpx = G == 1 ? 32 * kst : (G == 2 ? kst * 34 : kst * 36);      // x pixel slot of tap kx = 0 (G = 4: image pair)
                if (more) {
                    constexpr int NP = NXI + NDI, PER = (NP + NKS - 1) / NKS;
#pragma unroll
                    for (int q = 0; q < PER; ++q) {
                        const int pc = kk * PER + q;
                        if (pc < NDI) dma_dz(y + 1, pc);
                        else if (pc < NP) dma_x(y + 2, pc - NDI);
                    }
                }
                u32x4s Dh[2], Dm[2];                                           // dz fragments of the two output-channel halves
#pragma unroll
                for (int hd = 0; hd < 2; ++hd) {
                    Dh[hd] = swp_frag(ab + hd * HALF + dpx * 16);
                    Dm[hd] = NP == 2 ? swp_frag(ab + hd * HALF + (DZ_PART + dpx) * 16) : Dh[hd];
                }
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    // the three horizontal taps of a row read pixels 8 lg + kx .. + 7: ONE set of three transposed reads (12 pixels, six
                    // dwords of two pixels each) serves all three -- kx = 0: dwords 0-3, kx = 2: dwords 1-4, kx = 1: the 16-bit-shifted
                    // pairs (v_alignbit)
#pragma unroll
                    for (int hx = 0; hx < 2; ++hx) {
                        u32x4s Bs[2][3];
#pragma unroll
                        for (int pt = 0; pt < NP; ++pt) {
                            const unsigned ba = bb[ky] + hx * HALF + (pt * X_PART + xpx) * 16;
                            const u32x4s lo = swp_frag(ba);                                       // pixels 0 .. 7 of the lane's window
                            const s16x4w r2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4w*)(uintptr_t)(ba + 128));
                            const unsigned d4 = (unsigned)__builtin_bit_cast(unsigned long long, r2);   // pixels 8, 9
                            Bs[pt][0] = lo;
                            Bs[pt][1] = u32x4s{__builtin_amdgcn_alignbit(lo[1], lo[0], 16), __builtin_amdgcn_alignbit(lo[2], lo[1], 16),
                                               __builtin_amdgcn_alignbit(lo[3], lo[2], 16), __builtin_amdgcn_alignbit(d4, lo[3], 16)};
                            Bs[pt][2] = u32x4s{lo[1], lo[2], lo[3], d4};
                        }
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const u32x4s Xh = Bs[0][kx], Xm = NP == 2 ? Bs[1][kx] : Bs[0][kx];
                            const int t = ky * 3 + kx;
#pragma unroll
                            for (int hd = 0; hd < 2; ++hd) {
                                if constexpr (PM == 2) {
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, Xh), __builtin_bit_cast(bf16x8, Dh[hd]), acc[t][hx][hd], 0, 0, 0);
                                } else if constexpr (F16) {
                                    const f16x8 xh = __builtin_bit_cast(f16x8, Xh), xm = __builtin_bit_cast(f16x8, Xm);
                                    const f16x8 dh = __builtin_bit_cast(f16x8, Dh[hd]), dm = __builtin_bit_cast(f16x8, Dm[hd]);
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, dm, acc[t][hx][hd], 0, 0, 0);
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xm, dh, acc[t][hx][hd], 0, 0, 0);
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, dh, acc[t][hx][hd], 0, 0, 0);
                                } else {
                                    const bf16x8 xh = __builtin_bit_cast(bf16x8, Xh), xm = __builtin_bit_cast(bf16x8, Xm);
                                    const bf16x8 dh = __builtin_bit_cast(bf16x8, Dh[hd]), dm = __builtin_bit_cast(bf16x8, Dm[hd]);
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, dm, acc[t][hx][hd], 0, 0, 0);
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, dh, acc[t][hx][hd], 0, 0, 0);
                                    acc[t][hx][hd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, dh, acc[t][hx][hd], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        u += ye - yb;
    }

    float x_inv = 1.f, dz_inv = 1.f;
    const unsigned* xsl = (a.split_ch && ci0 >= a.split_ch) ? a.x_slots2 : a.x_slots;      // this block's 64 input channels
    (void)amax_scale(amax_read(xsl), false, x_inv);
    (void)amax_scale(amax_read(a.dz_slots), true, dz_inv);
    const float out_scale = (xsl ? x_inv : 1.f) * (a.dz_slots ? dz_inv : 1.f);
    const int64_t n = (int64_t)a.Cout * a.Cin;
    // lane: output channel co0 + 32 wm + 16 hd + r16, input channels ci0 + 32 wn + 16 hx + 4 lg .. + 3: one float4 (Cin % 8 == 0)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* o = a.slab + ((int64_t)(COT == 64 ? ks * 2 + grp : ks) * 9 + t) * n;
#pragma unroll
        for (int hx = 0; hx < 2; ++hx)
#pragma unroll
            for (int hd = 0; hd < 2; ++hd) {
                const int co = co0 + wm * 32 + 16 * hd + r16, ci = ci0 + wn * 32 + 16 * hx + 4 * lg;
                if (co < a.Cout && ci < a.Cin) *reinterpret_cast<f32x4s*>(o + (int64_t)co * a.Cin + ci) = acc[t][hx][hd] * out_scale;
            }
    }
}

int split_wgrad_group(int W) { return W >= 64 ? 1 : 64 / W; }      // images per unit: 1, 2 (W = 32), 4 (W = 16)

int split_wgrad_cot(int Cout, int W) { return (Cout % 128 == 0 && W >= 32) ? 128 : 64; }    // output channels per block

void split_wgrad_plan(int B, int Cin, int Cout, int H, int W, int& splitK, int& tilesX) {
    tilesX = W >= 64 ? cdiv(W, 64) : 1;
    const int64_t units = (int64_t)(B / split_wgrad_group(W)) * H * tilesX;
    const int tiles = cdiv(Cin, 64) * cdiv(Cout, split_wgrad_cot(Cout, W));
    int64_t k = std::max<int64_t>(1, device_cu_count() / tiles);    // one 4-wave block per CU (110 KB of LDS), one round
    k = std::min<int64_t>(k, std::max<int64_t>(1, units / 16));      // at least 16 rows per block
    splitK = (int)k;
}

}  // namespace

extern "C" {

int onet_conv3x3_split_wgrad_ok(int B, int Cin, int Cout, int H, int W) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0) return 0;
    if (W >= 64) return (W & 3) == 0 ? 1 : 0;
    return ((W == 32 || W == 16) && B % (64 / W) == 0) ? 1 : 0;         // narrower maps: 64 / W images side by side per unit
}

int64_t onet_conv3x3_split_wgrad_ws_bytes(int B, int Cin, int Cout, int H, int W) {
    int splitK, tx;
    split_wgrad_plan(B, Cin, Cout, H, W, splitK, tx);
    return (int64_t)splitK * (split_wgrad_cot(Cout, W) == 64 ? 2 : 1) * 9 * Cout * Cin * 4;    // 64-channel tiles: two K-groups per block, a slab each
}

static int split_wgrad_impl(const float* x, int64_t x_bs, const float* dz, int64_t dz_bs, float* dw, void* ws, int64_t ws_bytes,
                            int B, int Cin, int Cout, int H, int W, int accumulate, void* stream, const float* nsave, int n_groups,
                            int f16 = 0, const unsigned* x_amax = nullptr, const unsigned* dz_amax = nullptr) {
    ONET_REQUIRE(x && dz && dw && ws, "conv3x3_split_wgrad: null pointer");
    ONET_REQUIRE(!nsave || ((n_groups == 1 || n_groups == 2) && B % n_groups == 0),
                 "conv3x3_split_wgrad_norm: one or two statistics groups of equal size");
    ONET_REQUIRE(onet_conv3x3_split_wgrad_ok(B, Cin, Cout, H, W),
                 "conv3x3_split_wgrad: needs W >= 64 with W %% 4 == 0, or W = 32 / 16 with B %% (64 / W) == 0 (use onet_conv3x3_winograd_wgrad)");
    ONET_REQUIRE((x_bs & 3) == 0 && (dz_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(dz) & 15) == 0,
                 "conv3x3_split_wgrad: 16-byte aligned image rows required");
    ONET_REQUIRE(x_bs >= (int64_t)Cin * H * W && dz_bs >= (int64_t)Cout * H * W, "conv3x3_split_wgrad: batch stride too small");
    ONET_REQUIRE((int64_t)std::max(Cin, Cout) * H * W * 4 < (1ll << 31), "conv3x3_split_wgrad: image exceeds the 2 GiB buffer-resource range");
    const int G = split_wgrad_group(W);
    ONET_REQUIRE(G == 1 || (((int64_t)(B - 1) * x_bs + (int64_t)Cin * H * W) * 4 < (1ll << 31) &&
                            ((int64_t)(B - 1) * dz_bs + (int64_t)Cout * H * W) * 4 < (1ll << 31)),
                 "conv3x3_split_wgrad: on maps narrower than 64 pixels the whole batch must lie within the 2 GiB buffer-resource range");
    const int COT = split_wgrad_cot(Cout, W), slabs = COT == 64 ? 2 : 1;
    ONET_REQUIRE(!f16 || dz_amax, "conv3x3_split_wgrad_f16: the fp16 parts need the magnitude slots of dz");
    SwArgs a{x, x_bs, dz, dz_bs, (float*)ws, B, Cin, Cout, H, W, cdiv(Cin, 64), cdiv(Cout, COT), 1, 1, nsave, nsave ? B / n_groups : B,
             x_amax, dz_amax};
    split_wgrad_plan(B, Cin, Cout, H, W, a.splitK, a.tilesX);
    const int64_t need = (int64_t)a.splitK * slabs * 9 * Cout * Cin * 4;
    ONET_REQUIRE(ws_bytes >= need, "conv3x3_split_wgrad: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    const int64_t blocks = (int64_t)a.splitK * a.ciTiles * a.coTiles;
    const dim3 grid((unsigned)blocks), blk(512);
    hipStream_t st = as_stream(stream);
#define ONET_SW_LAUNCH(G_, COT_)                                                                                      \
    do {                                                                                                              \
        if (nsave && f16) hipLaunchKernelGGL((conv3x3_split_wgrad_kernel<G_, COT_, true, true>), grid, blk, 0, st, a);    \
        else if (nsave) hipLaunchKernelGGL((conv3x3_split_wgrad_kernel<G_, COT_, true, false>), grid, blk, 0, st, a);     \
        else if (f16) hipLaunchKernelGGL((conv3x3_split_wgrad_kernel<G_, COT_, false, true>), grid, blk, 0, st, a);       \
        else hipLaunchKernelGGL((conv3x3_split_wgrad_kernel<G_, COT_, false, false>), grid, blk, 0, st, a);               \
    } while (0)
    if (COT == 128) {
        if (G == 1) ONET_SW_LAUNCH(1, 128);
        else ONET_SW_LAUNCH(2, 128);
    } else if (G == 1) ONET_SW_LAUNCH(1, 64);
    else if (G == 2) ONET_SW_LAUNCH(2, 64);
    else ONET_SW_LAUNCH(4, 64);
#undef ONET_SW_LAUNCH
    int rc = check_launch("conv3x3_split_wgrad_kernel");
    if (rc) return rc;
    return launch_wgrad_reduce((const float*)ws, dw, a.splitK * slabs, 9, Cout, Cin, 0, accumulate, as_stream(stream));
}

int onet_conv3x3_split_wgrad(const float* x, int64_t x_bs, const float* dz, int64_t dz_bs, float* dw, void* ws, int64_t ws_bytes,
                             int B, int Cin, int Cout, int H, int W, int accumulate, void* stream) {
    return split_wgrad_impl(x, x_bs, dz, dz_bs, dw, ws, ws_bytes, B, Cin, Cout, H, W, accumulate, stream, nullptr, 0);
}

int onet_conv3x3_split_wgrad_norm(const float* z_prev, int64_t z_bs, const float* save, int n_groups, const float* dz, int64_t dz_bs,
                                  float* dw, void* ws, int64_t ws_bytes, int B, int Cin, int Cout, int H, int W, int accumulate,
                                  void* stream) {
    ONET_REQUIRE(save, "conv3x3_split_wgrad_norm: null pointer");
    return split_wgrad_impl(z_prev, z_bs, dz, dz_bs, dw, ws, ws_bytes, B, Cin, Cout, H, W, accumulate, stream, save, n_groups);
}

int onet_conv3x3_split_wgrad_pre_ok(int B, int Cin, int Cout, int H, int W) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || (Cin % 8) || (Cout % 8)) return 0;
    if (W >= 64) return 1;
    return ((W == 32 && B % 2 == 0) || (W == 16 && B % 4 == 0)) ? 1 : 0;
}

int onet_conv3x3_split_wgrad_pre(const void* xs, int64_t xs_bs, const void* x_amax, const void* x_amax2, int split_ch, const void* dzs,
                                 int64_t dzs_bs, const void* dz_amax, int f16, float* dw, void* ws, int64_t ws_bytes, int B, int Cin,
                                 int Cout, int H, int W, int accumulate, void* stream) {
    ONET_REQUIRE(split_ch >= 0 && split_ch < Cin && (split_ch % 64) == 0, "conv3x3_split_wgrad_pre: split_ch must be a multiple of 64 inside Cin");
    ONET_REQUIRE(xs && dzs && dw && ws, "conv3x3_split_wgrad_pre: null pointer");
    ONET_REQUIRE(onet_conv3x3_split_wgrad_pre_ok(B, Cin, Cout, H, W),
                 "conv3x3_split_wgrad_pre: needs Cin, Cout %% 8 == 0 and W >= 64, or W = 32 / 16 with a batch multiple of 2 / 4");
    ONET_REQUIRE((xs_bs & 3) == 0 && (dzs_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(xs) & 15) == 0 && (reinterpret_cast<uintptr_t>(dzs) & 15) == 0,
                 "conv3x3_split_wgrad_pre: 16-byte aligned slots required");
    ONET_REQUIRE(xs_bs >= (int64_t)Cin * H * W / (f16 == 2 ? 2 : 1) && dzs_bs >= (int64_t)Cout * H * W / (f16 == 2 ? 2 : 1),
                 "conv3x3_split_wgrad_pre: batch stride too small");
    ONET_REQUIRE((int64_t)std::max(Cin, Cout) * H * W * 4 < (1ll << 31), "conv3x3_split_wgrad_pre: image exceeds the 2 GiB buffer-resource range");
    const int G = split_wgrad_group(W);
    ONET_REQUIRE(G == 1 || (((int64_t)(B - 1) * xs_bs + (int64_t)Cin * H * W) * 4 < (1ll << 31) &&
                            ((int64_t)(B - 1) * dzs_bs + (int64_t)Cout * H * W) * 4 < (1ll << 31)),
                 "conv3x3_split_wgrad_pre: on 32-pixel maps the whole batch must lie within the 2 GiB buffer-resource range");
    const int COT = split_wgrad_cot(Cout, W), slabs = COT == 64 ? 2 : 1;
    SwPreArgs a{xs, xs_bs, dzs, dzs_bs, (float*)ws, B, Cin, Cout, H, W, cdiv(Cin, 64), cdiv(Cout, COT), 1, 1, (const unsigned*)x_amax,
                (const unsigned*)dz_amax, (const unsigned*)x_amax2, split_ch};
    split_wgrad_plan(B, Cin, Cout, H, W, a.splitK, a.tilesX);
    const int64_t need = (int64_t)a.splitK * slabs * 9 * Cout * Cin * 4;
    ONET_REQUIRE(ws_bytes >= need, "conv3x3_split_wgrad_pre: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    const int64_t blocks = (int64_t)a.splitK * a.ciTiles * a.coTiles;
    const dim3 grid((unsigned)blocks), blk(512);
    hipStream_t st = as_stream(stream);
    const int np = f16 == 2 ? 1 : 2, pxp = G == 4 ? 76 : SWP_PXP;
    const int lds = (4 * ((np * 8 * pxp + 63) / 64 * 64) + 2 * ((np * (COT / 8) * pxp + 63) / 64 * 64)) * 16;
#define ONET_SWP_LAUNCH(G_, COT_, F_)                                                                              \
    do {                                                                                                           \
        auto kern = conv3x3_wgrad_pre16_kernel<G_, COT_, F_>;                                                      \
        static PerDeviceOnce once;                                                                                 \
        if (once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
        hipLaunchKernelGGL(kern, grid, blk, lds, st, a);                                                           \
    } while (0)
#define ONET_SWP_F(G_, COT_) do { if (f16 == 2) ONET_SWP_LAUNCH(G_, COT_, 2); else if (f16) ONET_SWP_LAUNCH(G_, COT_, 1); else ONET_SWP_LAUNCH(G_, COT_, 0); } while (0)
    if (COT == 128) {
        if (G == 1) ONET_SWP_F(1, 128);
        else if (G == 2) ONET_SWP_F(2, 128);
        else ONET_SWP_F(4, 128);
    } else if (G == 1) ONET_SWP_F(1, 64);
    else if (G == 2) ONET_SWP_F(2, 64);
    else ONET_SWP_F(4, 64);
#undef ONET_SWP_F
#undef ONET_SWP_LAUNCH
    int rc = check_launch("conv3x3_split_wgrad_pre_kernel");
    if (rc) return rc;
    return launch_wgrad_reduce((const float*)ws, dw, a.splitK * slabs, 9, Cout, Cin, 0, accumulate, as_stream(stream));
}

int onet_conv3x3_split_pack_weights(const float* w, void* wq_fwd, void* wq_dgrad, void* amax_ws, int Cout, int Cin, int fwd_f16,
                                    int dgrad_f16, void* stream) {
    ONET_REQUIRE(w && (wq_fwd || wq_dgrad), "conv3x3_split_pack_weights: null pointer");
    ONET_REQUIRE(amax_ws || !(fwd_f16 == 1 || dgrad_f16 == 1), "conv3x3_split_pack_weights: the fp16 packs need the 8 KB magnitude workspace");
    if (fwd_f16 == 1 || dgrad_f16 == 1) {
        (void)hipMemsetAsync(amax_ws, 0, AMAX_SLOTS * AMAX_STRIDE * sizeof(unsigned), as_stream(stream));
        const int64_t nw = (int64_t)Cout * Cin * 9;
        hipLaunchKernelGGL(absmax_slots_kernel, dim3((unsigned)std::min<int64_t>((nw + 1023) / 1024, 1024)), dim3(256), 0, as_stream(stream), w,
                           nw, (unsigned*)amax_ws);
        int rc0 = check_launch("absmax_slots_kernel");
        if (rc0) return rc0;
    }
    ONET_REQUIRE(Cout > 0 && Cin > 0, "conv3x3_split_pack_weights: bad shape");
    ONET_REQUIRE(!wq_fwd || (Cin % 16) == 0, "conv3x3_split_pack_weights: the forward pack needs Cin %% 16 == 0");
    const int64_t n = (int64_t)std::max(Cin, ((Cout + 15) / 16) * 16) * 9 * std::max(Cin, Cout);
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 8192);
    if (wq_fwd) {
        hipLaunchKernelGGL(pack3x3_split_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), w, (__bf16*)wq_fwd, Cout, Cin, 0, fwd_f16,
                           (const unsigned*)amax_ws);
        int rc = check_launch("pack3x3_split_kernel");
        if (rc) return rc;
    }
    if (wq_dgrad) hipLaunchKernelGGL(pack3x3_split_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), w, (__bf16*)wq_dgrad, Cout, Cin, 1,
                                     dgrad_f16, (const unsigned*)amax_ws);
    return check_launch("pack3x3_split_kernel");
}

int onet_conv3x3_split_fwd(const float* x, int64_t x_bs, const void* wq, int wq_f16, float* z, int64_t z_bs, int B, int Cin, int Cout,
                           int H, int W, void* stream) {
    return split_fwd(x, x_bs, wq, z, z_bs, B, Cin, Cout, H, W, stream, nullptr, wq_f16);
}

int onet_absmax_slots(const float* x, int64_t n, void* slots, void* stream) {
    ONET_REQUIRE(x && slots && n > 0, "absmax_slots: bad args");
    hipLaunchKernelGGL(absmax_slots_kernel, dim3((unsigned)std::min<int64_t>((n + 1023) / 1024, 4096)), dim3(256), 0, as_stream(stream), x, n,
                       (unsigned*)slots);
    return check_launch("absmax_slots_kernel");
}

int onet_conv3x3_split_conv_amax(const float* x, int64_t x_bs, const void* x_amax, int scale_always, const void* wq, float* z, int64_t z_bs,
                                 float* part, int B, int Cin, int Cout, int H, int W, void* stream) {
    return split_fwd(x, x_bs, wq, z, z_bs, B, Cin, Cout, H, W, stream, part, 1, nullptr, 0, (const unsigned*)x_amax, scale_always);
}

int onet_conv3x3_split_wgrad_f16(const float* x, int64_t x_bs, const void* x_amax, const float* save, int n_groups, const float* dz,
                                 int64_t dz_bs, const void* dz_amax, float* dw, void* ws, int64_t ws_bytes, int B, int Cin, int Cout,
                                 int H, int W, int accumulate, void* stream) {
    return split_wgrad_impl(x, x_bs, dz, dz_bs, dw, ws, ws_bytes, B, Cin, Cout, H, W, accumulate, stream, save, save ? n_groups : 0, 1,
                            (const unsigned*)x_amax, (const unsigned*)dz_amax);
}

int onet_conv3x3_split_fwd_norm(const float* z_prev, int64_t z_bs, const float* save, int n_groups, const void* wq, int wq_f16,
                                const void* x_amax, float* z, int64_t zo_bs, float* part, int B, int Cin, int Cout, int H, int W,
                                void* stream) {
    ONET_REQUIRE(save, "conv3x3_split_fwd_norm: null pointer");
    return split_fwd(z_prev, z_bs, wq, z, zo_bs, B, Cin, Cout, H, W, stream, part, wq_f16, save, n_groups, (const unsigned*)x_amax);
}

int onet_split_pack_act(const float* x, int64_t x_bs, void* xs, int64_t xs_bs, int B, int C, int H, int W, int f16, float scale,
                        const void* slots, void* stream) {
    ONET_REQUIRE(x && xs, "split_pack_act: null pointer");
    ONET_REQUIRE(B > 0 && C > 0 && (C % 8) == 0 && H > 0 && W > 0, "split_pack_act: C must be a multiple of 8");
    ONET_REQUIRE((reinterpret_cast<uintptr_t>(xs) & 15) == 0 && (xs_bs & 3) == 0, "split_pack_act: 16-byte aligned slots required");
    const int64_t n = (int64_t)B * (C / 8) * H * W;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(split_pack_act_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), x, x_bs, (unsigned*)xs, xs_bs, B, C / 8, H, W,
                       f16, scale, (const unsigned*)slots);
    return check_launch("split_pack_act_kernel");
}

// The checks on the pre-split operand xs (activation or output gradient, batch stride xs_bs) and on the sizes that the four pre-split
// entries share: 0, or ONET_EINVAL with the entry's name in the message.  What is peculiar to one entry is checked there
static int pre_operand_checks(const char* entry, const void* xs, int64_t xs_bs, int wq_f16, int Cin, int Cout, int H, int W) {
    ONET_REQUIRE((Cin % (wq_f16 == 2 ? 32 : 16)) == 0, "%s: Cin must be a multiple of 16 (32 for plain bf16 operands)", entry);
    ONET_REQUIRE((xs_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(xs) & 15) == 0, "%s: 16-byte aligned slots required", entry);
    ONET_REQUIRE(xs_bs >= (int64_t)Cin * H * W / (wq_f16 == 2 ? 2 : 1), "%s: batch stride too small", entry);
    ONET_REQUIRE((int64_t)(Cin + 32) * H * W * 4 < (1ll << 31) && (int64_t)(Cin + 32) * 2 * 9 * Cout * 2 < (1ll << 31),
                 "%s: operand exceeds the 2 GiB buffer-resource range", entry);
    // 16-pixel maps: a tile's buffer resource spans an image pair
    ONET_REQUIRE(W != 16 || xs_bs * 4 + (int64_t)Cin * H * W * 4 < (1ll << 31), "%s: image pair exceeds the buffer-resource range", entry);
    return 0;
}

// BatchNorm statistics records of onet_conv3x3_split_fwd_pre: one per 16 x 32 tile; 16-pixel-wide maps: one per image PAIR and 16 rows
int onet_conv3x3_split_pre_nparts(int B, int H, int W) {
    if (W == 16) return (B > 0 && (B % 2) == 0 && (H % 16) == 0) ? (B / 2) * (H / 16) : 0;
    return split_nparts(B, H, W);
}

int onet_conv3x3_split_fwd_pre(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                               const void* wq, int wq_f16, void* z, int z_bf16, int64_t z_bs, float* part, int B, int Cin, int Cout, int H, int W,
                               void* stream) {
    ONET_REQUIRE(!z_bf16 || (wq_f16 == 2 && (z_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(z) & 7) == 0),
                 "conv3x3_split_fwd_pre: a bf16 output goes with plain bf16 operands (wq_f16 == 2), 8-byte aligned rows");
    ONET_REQUIRE(split_ch >= 0 && split_ch < Cin && (split_ch % 32) == 0, "conv3x3_split_fwd_pre: split_ch must be a multiple of 32 inside Cin");
    ONET_REQUIRE(xs && wq && z, "conv3x3_split_fwd_pre: null pointer");
    ONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && (W > 16 || (W == 16 && (B % 2) == 0 && (H % 16) == 0)),
                 "conv3x3_split_fwd_pre: bad shape (maps wider than 16 pixels, or exactly 16 wide with an even batch and H %% 16 == 0)");
    // plain bf16 operands take conv3x3_pre16_kernel at every width, and its epilogue stores whole 4-pixel vectors of a row
    ONET_REQUIRE(wq_f16 != 2 || (W % 4) == 0, "conv3x3_split_fwd_pre: plain bf16 operands need W %% 4 == 0");
    if (const int rc = pre_operand_checks("conv3x3_split_fwd_pre", xs, xs_bs, wq_f16, Cin, Cout, H, W)) return rc;
    ONET_REQUIRE(z_bs >= (int64_t)Cout * H * W, "conv3x3_split_fwd_pre: batch stride too small");
    SpPreArgs a{xs, xs_bs, (const __bf16*)wq, (float*)z, z_bs, B, Cin, Cout, H, W, 0, 0, 0, part, (const unsigned*)x_amax, scale_always,
                (const unsigned*)x_amax2, split_ch};
    a.z16 = z_bf16 ? 1 : 0;
    if (part) ONET_REQUIRE(onet_conv3x3_split_pre_nparts(B, H, W) > 0, "conv3x3_split_fwd_pre: statistics need a map made of full 16 x 32 tiles");
    hipStream_t st = as_stream(stream);
    if (W == 16) {
        if (wq_f16 == 2) return part ? launch_split_pre<true, 2, true>(a, st) : launch_split_pre<false, 2, true>(a, st);
        if (wq_f16) return part ? launch_split_pre<true, 1, true>(a, st) : launch_split_pre<false, 1, true>(a, st);
        return part ? launch_split_pre<true, 0, true>(a, st) : launch_split_pre<false, 0, true>(a, st);
    }
    if (wq_f16 == 2) return part ? launch_split_pre<true, 2, false>(a, st) : launch_split_pre<false, 2, false>(a, st);
    if (wq_f16) return part ? launch_split_pre<true, 1, false>(a, st) : launch_split_pre<false, 1, false>(a, st);
    return part ? launch_split_pre<true, 0, false>(a, st) : launch_split_pre<false, 0, false>(a, st);
}

// Input gradient of the SECOND convolution of a DoubleConv from pre-split dz, with the BatchNorm-backward reduce pass of the FIRST unit
// (whose output gradient this launch produces) in the epilogue: see SpPreArgs::rd_*.  Returns 1 (nothing launched) where the map is not
// made of full tiles.  rec4: [onet_conv3x3_split_pre_nparts(B, H, W)][Cout][4] floats.
int onet_conv3x3_split_dgrad_pre_bnreduce(const void* dzs, int64_t dzs_bs, const void* dz_amax, int scale_always, const void* wq, int wq_f16,
                                          float* da, int64_t da_bs, const void* z_prev, int z_bf16, int64_t z_bs, const float* save, int group_images,
                                          float* rec4, void* da_amax, int B, int Cin, int Cout, int H, int W, void* stream) {
    ONET_REQUIRE(dzs && wq && da && z_prev && save && rec4, "conv3x3_split_dgrad_pre_bnreduce: null pointer");
    if (onet_conv3x3_split_pre_nparts(B, H, W) <= 0 || (W != 16 && (W % 32)) || (Cout % 16)) return 1;
    if (W == 16 && ((group_images % 2) || wq_f16 != 2)) return 1;    // a tile's image pair must lie in one statistics group; (hi | mid)
                                                                     // parts on 16-pixel maps: not built (register budget of that instance)
    // a tile of fewer than four chunks is too short to cover the epilogue's z loads (plain bf16 operands, 64 channels of dz: two chunks --
    // measured at BASELINE configs[2]: the fused launches cost more than the reduce pass they replace)
    if (Cin / (wq_f16 == 2 ? 32 : 16) < 4) return 1;
    ONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0, "conv3x3_split_dgrad_pre_bnreduce: bad shape");
    ONET_REQUIRE(group_images >= 0 && (group_images == 0 || B % group_images == 0), "conv3x3_split_dgrad_pre_bnreduce: bad statistics groups");
    if (const int rc = pre_operand_checks("conv3x3_split_dgrad_pre_bnreduce", dzs, dzs_bs, wq_f16, Cin, Cout, H, W)) return rc;
    ONET_REQUIRE((z_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(z_prev) & (z_bf16 ? 7 : 15)) == 0 && (da_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(da) & 15) == 0,
                 "conv3x3_split_dgrad_pre_bnreduce: 16-byte aligned rows required");
    ONET_REQUIRE(da_bs >= (int64_t)Cout * H * W && z_bs >= (int64_t)Cout * H * W, "conv3x3_split_dgrad_pre_bnreduce: batch stride too small");
    SpPreArgs a{dzs, dzs_bs, (const __bf16*)wq, da, da_bs, B, Cin, Cout, H, W, 0, 0, 0, nullptr, (const unsigned*)dz_amax, scale_always, nullptr, 0};
    a.rd_z = (const float*)z_prev;
    a.rd_z16 = z_bf16 ? 1 : 0;
    a.rd_z_bs = z_bs;
    a.rd_save = save;
    a.rd_gimg = group_images;
    a.rd_rec = rec4;
    a.rd_amax = (unsigned*)da_amax;
    hipStream_t st = as_stream(stream);
    if (W == 16) return launch_split_pre<false, 2, true, true>(a, st);
    if (wq_f16 == 2) return launch_split_pre<false, 2, false, true>(a, st);
    return wq_f16 ? launch_split_pre<false, 1, false, true>(a, st) : launch_split_pre<false, 0, false, true>(a, st);
}

// Input gradient of a decoder block's FIRST convolution (fp16 hi | mid parts): channels < ch0 of da as fp32, channels >= ch0 -- the
// up-sampled half of the concat gradient, read only by the ConvTranspose2d backward GEMMs -- pre-split into daP (SpPreArgs::zP).
int onet_conv3x3_split_dgrad_pre_slots(const void* dzs, int64_t dzs_bs, const void* dz_amax, int scale_always, const void* wq, int wq_f16,
                                       float* da, int64_t da_bs, void* daP, int64_t daP_bs, int ch0, const void* daP_amax, int B, int Cin,
                                       int Cout, int H, int W, void* stream) {
    ONET_REQUIRE(dzs && wq && da && daP && (daP_amax || wq_f16 == 2) && (wq_f16 == 1 || wq_f16 == 2), "conv3x3_split_dgrad_pre_slots: bad args");
    ONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W >= 32 && (W % 32) == 0 && (H % 16) == 0,
                 "conv3x3_split_dgrad_pre_slots: maps made of full 16 x 32 tiles");
    ONET_REQUIRE(ch0 > 0 && ch0 < Cout && (ch0 % 64) == 0 && (Cout % 64) == 0, "conv3x3_split_dgrad_pre_slots: ch0 and Cout must be multiples of 64");
    if (const int rc = pre_operand_checks("conv3x3_split_dgrad_pre_slots", dzs, dzs_bs, wq_f16, Cin, Cout, H, W)) return rc;
    ONET_REQUIRE((daP_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(daP) & 15) == 0, "conv3x3_split_dgrad_pre_slots: 16-byte aligned slots required");
    ONET_REQUIRE(da_bs >= (int64_t)ch0 * H * W && daP_bs >= (int64_t)(Cout - ch0) * H * W / (wq_f16 == 2 ? 2 : 1),
                 "conv3x3_split_dgrad_pre_slots: batch stride too small");
    SpPreArgs a{dzs, dzs_bs, (const __bf16*)wq, da, da_bs, B, Cin, Cout, H, W, 0, 0, 0, nullptr, (const unsigned*)dz_amax, scale_always, nullptr, 0};
    a.zP = daP;
    a.zP_bs = daP_bs;
    a.zP_ch0 = ch0;
    a.zP_slots = (const unsigned*)daP_amax;
    if (wq_f16 == 2) return launch_split_pre<false, 2, false>(a, as_stream(stream));      // plain bf16: one part, unscaled (conv3x3_pre16_kernel)
    return launch_split_pre<false, 1, false>(a, as_stream(stream));
}

// ----------------------------------------------------------------------------- eval-mode inference (onet_amd/inference.py)
// The eighteen entries below are points of one small space -- slot format x map mode x epilogue -- and share one checked launch path,
// eval_conv: each entry is a descriptor row and its arguments.  A new format, mode or epilogue is a row here (and DESIGN.md, "The fused
// eval table", names the other places).
//
// Slot format (EvalEntry::parts).  2: fp16 (hi | mid) parts, the forward convolution of onet_conv3x3_split_fwd_pre(wq_f16 = 1); the
// activation leaves as aP [B][Cout/8][H][2][W][8] = parts of 2^k relu(bn(z)), k by the guard rule from the bound aP_slots holds BEFORE
// the launch (onet_conv3x3_act_bound); x_amax / scale_always / x_amax2 / split_ch: the operand's magnitude slots, as there.  1: ONE part
// of plain bf16 (wq_f16 = 2), unscaled -- bf16 has fp32's exponent range, so no magnitude slots, bound or guard: aP [B][Cout/8][H][W][8]
// bf16 (round to nearest even).  Batch strides in 4-byte units (the leading channel groups of a concat buffer qualify).
//
// Map mode (EvMap): the maps an entry takes; outside them 1, nothing launched.
//   Full    maps made of full 16 x 32 tiles.
//   Ragged  any map of even H and W % 4 == 0 below 2^24 pixels (include/onet_hip_ragged.h, onet_hip_ragged_split.h): the tile counts are
//           cdiv, the staging gives every out-of-map slot the out-of-range offset and every store is guarded per slot / float4 / pooled
//           float2; with H and W even and tiles starting on even coordinates a 2 x 2 pooling window is wholly inside the map or wholly
//           outside.  On the map, value for value, what the full-tile entry writes on the map zero-padded to whole tiles; nothing outside
//           it is written.  A map of full tiles takes the full-tile instance: the same launch, the same bits.  The exact-maximum record
//           of the one-part activation epilogue covers a tile's out-of-map accumulators too, so the one-part ragged entries take no
//           a_amax (an error); the fp16 instances mask their record to the MAP's pixels and take it.
//   AnyMap  ANY H and W (include/onet_hip_anymap.h; one-part operands): the levels below the first of an input such as 200 x 200 (50 x 50:
//           W % 4 == 2; 25 x 25: odd).  Domain: H W < 2^24, Cin % 32 == 0, Cout % 64 == 0, inside the buffer-resource range, a_amax NULL.
//           A map the ragged entry takes goes to that entry's path, under this entry's name; every other map to the ANY instance, whose
//           fp32 side outputs are stored float by float (4-byte alignment of a / y is enough).  The pooled maps are H / 2 x W / 2 rounded
//           DOWN (nn.MaxPool2d(2)), and the stride checks use those sizes.
//   Pairs   IMAGE-PAIR tiles (include/onet_hip_pairs.h, onet_hip_split_pairs.h): maps of any H and 0 < W <= 16 -- the bottom level of the
//           eval plan (16 x 16, 14 x 14, 12 x 12) -- two images side by side in a tile's 32 columns, each with its own halo columns
//           (SpPreCfg<true>), where the any-map / ragged entry walks one half-empty tile per image.  On the map, value for value, what that
//           entry writes: the same chunks and taps in the same order per pixel, the same epilogue expressions, the same 2^k.  Any batch
//           size: the last tile of an odd one holds one image (masked in the fp16 instance's a_amax record like an out-of-map pixel).
//           1 also for an image pair beyond the buffer-resource range (a tile's buffer resource spans the batch stride, then one image and
//           the chunk the staging runs ahead by); the one-part entry: for a non-NULL a_amax too.
//
// Epilogue (EvEpi).
//   Act    a FIXED BatchNorm + ReLU of `save` [4][Cout] (onet_bn_eval_coeffs) on the accumulators, the activation leaving as slots
//          (SpPreArgs::act_*).  a_amax (may be NULL): magnitude slots that receive the exact max a; a (may be NULL): the activation as fp32
//          NCHW too.  Bit for bit what the plain launch followed by onet_bn_relu_apply_split writes; z itself is never stored.
//   Pool   an encoder block's second unit: Act with the 2 x 2 max-pooling of the activation in the same epilogue (SpPreArgs::pl_*).
//          Everything Act writes is written as it writes it, plus the pooled tensor m = max over each 2 x 2 window of relu(bn(z)): as slots
//          yP [B][Cout/8][H/2][parts][W/2][8] (fp16: the parts of 2^k m with aP's k), as fp32 y [B][Cout][H/2][W/2], or both; at least
//          one.  Bit for bit what the plain launch followed by onet_bn_relu_apply_pool_split writes.
//   Head   labels-only inference, the model's LAST unit (SpPreArgs::hd_*): h = max(0, fma(z - mean, sc, sh)) on the accumulators and
//          V [B][H][W] = sum_c L[c] h[c] (L: fp32 NCHW, batch stride L_bs) -- nothing else is stored.  Cout == 64, else 1.
//   Plain  the plain forward (fp32 z, no statistics) on a ragged map: the plan's last unit where no head epilogue follows.
enum class EvMap { Full, Ragged, AnyMap, Pairs };
enum class EvEpi { Act, Pool, Head, Plain };
struct EvalEntry {
    const char* name;      // what the messages start with
    int parts;             // operand kind: 1 (plain bf16) or 2 (fp16 hi | mid)
    EvMap map;
    EvEpi epi;
};
// The arguments of an entry, grouped as the prototypes list them; a group the entry does not have stays empty
struct EvSlots { const void* x_amax = nullptr; int scale_always = 0; const void* x_amax2 = nullptr; int split_ch = 0; };
struct EvAct { void* aP = nullptr; int64_t aP_bs = 0; const void* aP_slots = nullptr; void* a_amax = nullptr; float* a = nullptr; int64_t a_bs = 0; };
struct EvPool { void* yP = nullptr; int64_t yP_bs = 0; float* y = nullptr; int64_t y_bs = 0; };
struct EvHead { const float* L = nullptr; int64_t L_bs = 0; float* V = nullptr; };
struct EvPlain { float* z = nullptr; int64_t z_bs = 0; };
struct EvalConv {
    const void* xs;
    int64_t xs_bs;
    EvSlots in;
    const void* wq;
    const float* save;
    EvAct act;
    EvPool pool;
    EvHead head;
    EvPlain plain;
    int B, Cin, Cout, H, W;
    void* stream;
};

static bool pre_map_ok(bool ragged, int H, int W) {
    if (ragged) return !((H & 1) || (W & 3) || (int64_t)H * W >= (1 << 24));
    return !(W < 32 || (W % 32) || (H % 16));
}

// (p may be NULL; bs: its batch stride, a multiple of 4 where rows are read as vectors -- 0 where it does not matter)
static bool aligned(const void* p, int64_t bs, int bytes) { return !p || ((bs & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0); }

static int eval_conv(const EvalEntry& e, const EvalConv& g) {
    const char* entry = e.name;
    const bool one = e.parts == 1, pool = e.epi == EvEpi::Pool, act = pool || e.epi == EvEpi::Act;
    const int B = g.B, Cin = g.Cin, Cout = g.Cout, H = g.H, W = g.W;
    // 1. null pointers
    if (act) ONET_REQUIRE(g.xs && g.wq && g.save && g.act.aP && (g.act.aP_slots || one), "%s: null pointer", entry);
    else if (e.epi == EvEpi::Head) ONET_REQUIRE(g.xs && g.wq && g.save && g.head.L && g.head.V, "%s: null pointer", entry);
    else ONET_REQUIRE(g.xs && g.wq && g.plain.z, "%s: null pointer", entry);
    ONET_REQUIRE(!pool || g.pool.yP || g.pool.y, "%s: a pooled destination is required (yP, y or both)", entry);
    // 2. shape
    ONET_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: bad shape", entry);
    // 3. domain: 1, nothing launched
    const int64_t image = (int64_t)(Cin + 32) * H * W * 4, pack = (int64_t)(Cin + 32) * 2 * 9 * Cout * 2;      // bytes in a buffer resource
    EvMap map = e.map;
    if ((Cin % (one ? 32 : 16)) || (e.epi == EvEpi::Head ? Cout != 64 : (Cout % 64))) return 1;
    if (map == EvMap::AnyMap || map == EvMap::Pairs) {
        // (the other entries report an operand beyond the range as an error, pre_operand_checks; the fp16 pair entry: its image too)
        if (pack >= (1ll << 31) || (one && (g.act.a_amax || (int64_t)H * W >= (1 << 24) || image >= (1ll << 31)))) return 1;
        if (map == EvMap::Pairs && (W > 16 || g.xs_bs > (1ll << 29) || g.xs_bs * 4 + image >= (1ll << 31))) return 1;
        if (map == EvMap::AnyMap && pre_map_ok(true, H, W)) map = EvMap::Ragged;
    } else if (!pre_map_ok(map == EvMap::Ragged, H, W)) {
        return 1;
    }
    // 4. argument checks
    ONET_REQUIRE(!(one && map == EvMap::Ragged) || !g.act.a_amax, "%s: the ragged entry records no exact maximum (a_amax must be NULL)", entry);
    ONET_REQUIRE(g.in.split_ch >= 0 && g.in.split_ch < Cin && (g.in.split_ch % 32) == 0, "%s: split_ch must be a multiple of 32 inside Cin", entry);
    if (const int rc = pre_operand_checks(entry, g.xs, g.xs_bs, one ? 2 : 1, Cin, Cout, H, W)) return rc;
    const int64_t n = (int64_t)Cout * H * W, np = (int64_t)Cout * (H >> 1) * (W >> 1), per = one ? 2 : 1;      // per: slot elements per 4-byte unit
    if (act) {
        ONET_REQUIRE(aligned(g.act.aP, g.act.aP_bs, 16) && aligned(g.pool.yP, g.pool.yP_bs, 16), "%s: 16-byte aligned slots required", entry);
        if (map == EvMap::AnyMap || map == EvMap::Pairs)
            ONET_REQUIRE(aligned(g.act.a, 0, 4) && aligned(g.pool.y, 0, 4), "%s: 4-byte aligned floats required", entry);
        else if (one || pool)      // (the fp16 Act entries on whole images have never asked this of `a`)
            ONET_REQUIRE(aligned(g.act.a, g.act.a_bs, 16) && aligned(g.pool.y, g.pool.y_bs, 16), "%s: 16-byte aligned rows required", entry);
        ONET_REQUIRE(g.act.aP_bs >= n / per && (!g.act.a || g.act.a_bs >= n) && (!g.pool.yP || g.pool.yP_bs >= np / per) && (!g.pool.y || g.pool.y_bs >= np),
                     "%s: batch stride too small", entry);
    } else if (e.epi == EvEpi::Head) {
        ONET_REQUIRE(aligned(g.head.L, g.head.L_bs, 16) && aligned(g.head.V, 0, 16), "%s: 16-byte aligned rows required", entry);
        ONET_REQUIRE(g.head.L_bs >= n, "%s: batch stride too small", entry);
    } else {
        ONET_REQUIRE(aligned(g.plain.z, g.plain.z_bs, 16), "%s: 16-byte aligned rows required", entry);
        ONET_REQUIRE(g.plain.z_bs >= n, "%s: batch stride too small", entry);
    }
    SpPreArgs p{g.xs, g.xs_bs, (const __bf16*)g.wq, g.plain.z, g.plain.z_bs, B, Cin, Cout, H, W, 0, 0, 0, nullptr, (const unsigned*)g.in.x_amax,
                g.in.scale_always, (const unsigned*)g.in.x_amax2, g.in.split_ch};
    p.act_save = g.save;
    if (act) {
        p.zP = g.act.aP;
        p.zP_bs = g.act.aP_bs;
        p.zP_ch0 = 0;
        p.zP_slots = (const unsigned*)g.act.aP_slots;
        p.act_amax = (unsigned*)g.act.a_amax;
        p.act_a = g.act.a;
        p.act_a_bs = g.act.a_bs;
    }
    if (pool) {
        p.pl_P = g.pool.yP;
        p.pl_P_bs = g.pool.yP_bs;
        p.pl_y = g.pool.y;
        p.pl_y_bs = g.pool.y_bs;
    } else if (e.epi == EvEpi::Head) {
        p.hd_L = g.head.L;
        p.hd_L_bs = g.head.L_bs;
        p.hd_V = g.head.V;
    }
    // the instances that exist: <ST, PM, W16, RD, ACT, HEAD, POOL, RAG, ANY>.  A map of full tiles takes the full-tile instance from every entry
    hipStream_t st = as_stream(g.stream);
    const bool pairs = map == EvMap::Pairs, any = map == EvMap::AnyMap, rag = map == EvMap::Ragged && !pre_map_ok(false, H, W);
    if (one) {
        if (e.epi == EvEpi::Plain) return launch_split_pre<false, 2, false>(p, st);
        if (e.epi == EvEpi::Head) return launch_split_pre<false, 2, false, false, false, true>(p, st);
        if (pool && any) return launch_split_pre<false, 2, false, false, true, false, true, false, true>(p, st);
        if (pool && rag) return launch_split_pre<false, 2, false, false, true, false, true, true>(p, st);
        if (pool) return launch_split_pre<false, 2, false, false, true, false, true>(p, st);
        if (pairs) return launch_split_pre<false, 2, true, false, true>(p, st);
        if (any) return launch_split_pre<false, 2, false, false, true, false, false, false, true>(p, st);
        return launch_split_pre<false, 2, false, false, true>(p, st);       // (Act: one instance on full tiles and ragged maps)
    }
    if (e.epi == EvEpi::Plain) return launch_split_pre<false, 1, false>(p, st);
    if (e.epi == EvEpi::Head) return launch_split_pre<false, 1, false, false, false, true>(p, st);
    if (pool && rag) return launch_split_pre<false, 1, false, false, true, false, true, true>(p, st);
    if (pool) return launch_split_pre<false, 1, false, false, true, false, true>(p, st);
    if (pairs) return launch_split_pre<false, 1, true, false, true, false, false, true>(p, st);
    if (rag) return launch_split_pre<false, 1, false, false, true, false, false, true>(p, st);
    return launch_split_pre<false, 1, false, false, true>(p, st);
}

int onet_conv3x3_split_fwd_pre_act(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                   const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots, void* a_amax, float* a,
                                   int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_act", 2, EvMap::Full, EvEpi::Act}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq, save,
                     {aP, aP_bs, aP_slots, a_amax, a, a_bs}, {}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_act_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                          const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots, void* a_amax, float* a,
                                          int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_act_ragged", 2, EvMap::Ragged, EvEpi::Act}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq, save,
                     {aP, aP_bs, aP_slots, a_amax, a, a_bs}, {}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_act_pairs(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                         const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots, void* a_amax, float* a,
                                         int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_act_pairs", 2, EvMap::Pairs, EvEpi::Act}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq, save,
                     {aP, aP_bs, aP_slots, a_amax, a, a_bs}, {}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_plain_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                            const void* wq, float* z, int64_t z_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_plain_ragged", 2, EvMap::Ragged, EvEpi::Plain}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq,
                     nullptr, {}, {}, {}, {z, z_bs}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_act_pool(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                        const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots, void* a_amax, float* a,
                                        int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B, int Cin, int Cout, int H, int W,
                                        void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_act_pool", 2, EvMap::Full, EvEpi::Pool}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq, save,
                     {aP, aP_bs, aP_slots, a_amax, a, a_bs}, {yP, yP_bs, y, y_bs}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_act_pool_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2,
                                               int split_ch, const void* wq, const float* save, void* aP, int64_t aP_bs, const void* aP_slots,
                                               void* a_amax, float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B, int Cin,
                                               int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_act_pool_ragged", 2, EvMap::Ragged, EvEpi::Pool}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq,
                     save, {aP, aP_bs, aP_slots, a_amax, a, a_bs}, {yP, yP_bs, y, y_bs}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_head(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                    const void* wq, const float* save, const float* L, int64_t L_bs, float* V, int B, int Cin, int Cout, int H,
                                    int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_head", 2, EvMap::Full, EvEpi::Head}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq, save, {}, {},
                     {L, L_bs, V}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_split_fwd_pre_head_ragged(const void* xs, int64_t xs_bs, const void* x_amax, int scale_always, const void* x_amax2, int split_ch,
                                           const void* wq, const float* save, const float* L, int64_t L_bs, float* V, int B, int Cin, int Cout,
                                           int H, int W, void* stream) {
    return eval_conv({"conv3x3_split_fwd_pre_head_ragged", 2, EvMap::Ragged, EvEpi::Head}, {xs, xs_bs, {x_amax, scale_always, x_amax2, split_ch}, wq, save,
                     {}, {}, {L, L_bs, V}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs, void* a_amax,
                                     float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act", 1, EvMap::Full, EvEpi::Act}, {xs, xs_bs, {}, wq, save, {aP, aP_bs, nullptr, a_amax, a, a_bs}, {}, {}, {},
                     B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act_ragged(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                            void* a_amax, float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act_ragged", 1, EvMap::Ragged, EvEpi::Act}, {xs, xs_bs, {}, wq, save, {aP, aP_bs, nullptr, a_amax, a, a_bs}, {},
                     {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act_anymap(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                            void* a_amax, float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act_anymap", 1, EvMap::AnyMap, EvEpi::Act}, {xs, xs_bs, {}, wq, save, {aP, aP_bs, nullptr, a_amax, a, a_bs}, {},
                     {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act_pairs(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                           void* a_amax, float* a, int64_t a_bs, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act_pairs", 1, EvMap::Pairs, EvEpi::Act}, {xs, xs_bs, {}, wq, save, {aP, aP_bs, nullptr, a_amax, a, a_bs}, {},
                     {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_plain_ragged(const void* xs, int64_t xs_bs, const void* wq, float* z, int64_t z_bs, int B, int Cin, int Cout,
                                              int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_plain_ragged", 1, EvMap::Ragged, EvEpi::Plain}, {xs, xs_bs, {}, wq, nullptr, {}, {}, {}, {z, z_bs}, B, Cin,
                     Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act_pool(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs, void* a_amax,
                                          float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B, int Cin, int Cout, int H,
                                          int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act_pool", 1, EvMap::Full, EvEpi::Pool}, {xs, xs_bs, {}, wq, save, {aP, aP_bs, nullptr, a_amax, a, a_bs},
                     {yP, yP_bs, y, y_bs}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act_pool_ragged(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                                 void* a_amax, float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B,
                                                 int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act_pool_ragged", 1, EvMap::Ragged, EvEpi::Pool}, {xs, xs_bs, {}, wq, save,
                     {aP, aP_bs, nullptr, a_amax, a, a_bs}, {yP, yP_bs, y, y_bs}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_act_pool_anymap(const void* xs, int64_t xs_bs, const void* wq, const float* save, void* aP, int64_t aP_bs,
                                                 void* a_amax, float* a, int64_t a_bs, void* yP, int64_t yP_bs, float* y, int64_t y_bs, int B,
                                                 int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_act_pool_anymap", 1, EvMap::AnyMap, EvEpi::Pool}, {xs, xs_bs, {}, wq, save,
                     {aP, aP_bs, nullptr, a_amax, a, a_bs}, {yP, yP_bs, y, y_bs}, {}, {}, B, Cin, Cout, H, W, stream});
}

int onet_conv3x3_plain16_fwd_pre_head(const void* xs, int64_t xs_bs, const void* wq, const float* save, const float* L, int64_t L_bs, float* V,
                                      int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_head", 1, EvMap::Full, EvEpi::Head}, {xs, xs_bs, {}, wq, save, {}, {}, {L, L_bs, V}, {}, B, Cin, Cout, H, W,
                     stream});
}

int onet_conv3x3_plain16_fwd_pre_head_ragged(const void* xs, int64_t xs_bs, const void* wq, const float* save, const float* L, int64_t L_bs,
                                             float* V, int B, int Cin, int Cout, int H, int W, void* stream) {
    return eval_conv({"conv3x3_plain16_fwd_pre_head_ragged", 1, EvMap::Ragged, EvEpi::Head}, {xs, xs_bs, {}, wq, save, {}, {}, {L, L_bs, V}, {}, B, Cin, Cout,
                     H, W, stream});
}

// a[co] = relu(sc (z - mean) + sh) with |z[co]| <= sum_ci |w[co][ci][.]| max |x[ci]|:  |a[co]| <= |sc| (S1 max1 + S2 max2) + |sh - mean sc|,
// S1 / S2 = the L1 norms of the output channel's weights over the input channels below / from split_ch, max1 / max2 the two producers'
// magnitudes (x_amax, x_amax2; one group: split_ch = 0).  The largest over co goes into out_slots (zeroed by the caller): the bound
// onet_conv3x3_split_fwd_pre_act scales its slots by -- evaluated in fp64 and rounded UP to fp32.  save: [4][Cout], bn_eval_coeffs' format
__global__ __launch_bounds__(256) void conv3x3_act_bound_kernel(const float* __restrict__ w, int Cout, int Cin, const float* __restrict__ save,
                                                                const unsigned* __restrict__ x_slots, const unsigned* __restrict__ x_slots2,
                                                                int split_ch, unsigned* __restrict__ out_slots) {
    __shared__ double red[2][4];
    const double m1 = (double)amax_read(x_slots), m2 = x_slots2 ? (double)amax_read(x_slots2) : m1;
    const int co = blockIdx.x;
    const int n1 = (x_slots2 && split_ch > 0 ? split_ch : Cin) * 9;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < Cin * 9; i += 256) {
        const double v = (double)fabsf(w[(int64_t)co * Cin * 9 + i]);
        if (i < n1) s1 += v;
        else s2 += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s1;
        red[1][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double S1 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), S2 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double mean = save[co], sc = save[2 * Cout + co], sh = save[3 * Cout + co];
        const double bound = fabs(sc) * (S1 * m1 + S2 * m2) + fabs(sh - mean * sc);
        float f = (float)bound;
        if ((double)f < bound) f = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, f) + 1u);      // round up (f >= 0, finite)
        if (f == f) atomicMax(out_slots + (blockIdx.x & (AMAX_SLOTS - 1)) * AMAX_STRIDE, __builtin_bit_cast(unsigned, f));
    }
}

int onet_conv3x3_act_bound(const float* w, int Cout, int Cin, const float* save, const void* x_amax, const void* x_amax2, int split_ch,
                           void* out_slots, void* stream) {
    ONET_REQUIRE(w && save && x_amax && out_slots && Cout > 0 && Cin > 0, "conv3x3_act_bound: bad args");
    ONET_REQUIRE(split_ch >= 0 && split_ch < Cin && (x_amax2 || split_ch == 0), "conv3x3_act_bound: split_ch must lie inside Cin and go with x_amax2");
    hipLaunchKernelGGL(conv3x3_act_bound_kernel, dim3((unsigned)Cout), dim3(256), 0, as_stream(stream), w, Cout, Cin, save,
                       (const unsigned*)x_amax, (const unsigned*)x_amax2, split_ch, (unsigned*)out_slots);
    return check_launch("conv3x3_act_bound_kernel");
}

// |da[ci]| <= max |dz| * sum over (co, tap) of |w[co][ci][tap]|: the bound of the input gradient's channels >= ci0 from the bound of dz
// (dz_amax) and the weights, into out_slots (zeroed by the caller) -- what onet_conv3x3_split_dgrad_pre_slots scales its slots by
__global__ __launch_bounds__(256) void conv3x3_dgrad_bound_kernel(const float* __restrict__ w, int Cout, int Cin, int ci0,
                                                                  const unsigned* __restrict__ dz_slots, unsigned* __restrict__ out_slots) {
    __shared__ float red[4];
    const float dzmax = amax_read(dz_slots);
    const int ci = ci0 + blockIdx.x;
    float sm = 0.f;
    for (int i = threadIdx.x; i < Cout * 9; i += 256) sm += fabsf(w[((int64_t)(i / 9) * Cin + ci) * 9 + i % 9]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sm;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float bound = ((red[0] + red[1]) + (red[2] + red[3])) * dzmax * 1.00001f;
        if (bound == bound) atomicMax(out_slots + (blockIdx.x & (AMAX_SLOTS - 1)) * AMAX_STRIDE, __builtin_bit_cast(unsigned, bound));
    }
}

int onet_conv3x3_dgrad_bound(const float* w, int Cout, int Cin, int ci0, const void* dz_amax, void* out_slots, void* stream) {
    ONET_REQUIRE(w && dz_amax && out_slots && Cout > 0 && ci0 >= 0 && ci0 < Cin, "conv3x3_dgrad_bound: bad args");
    hipLaunchKernelGGL(conv3x3_dgrad_bound_kernel, dim3((unsigned)(Cin - ci0)), dim3(256), 0, as_stream(stream), w, Cout, Cin, ci0,
                       (const unsigned*)dz_amax, (unsigned*)out_slots);
    return check_launch("conv3x3_dgrad_bound_kernel");
}

int onet_conv3x3_split_nparts(int B, int H, int W) { return split_nparts(B, H, W); }

int onet_conv3x3_split_fwd_stats(const float* x, int64_t x_bs, const void* wq, int wq_f16, float* z, int64_t z_bs, float* part, int B,
                                 int Cin, int Cout, int H, int W, void* stream) {
    ONET_REQUIRE(part, "conv3x3_split_fwd_stats: null pointer");
    return split_fwd(x, x_bs, wq, z, z_bs, B, Cin, Cout, H, W, stream, part, wq_f16);
}

}  // extern "C"
