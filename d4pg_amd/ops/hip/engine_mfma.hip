// f32 MFMA GEMM kernels (v_mfma_f32_32x32x2_f32 — exact fp32 at the full fp32
// rate): forward, dX and split-K dW on 64x128 workgroup tiles with double-
// buffered LDS K-slices, plus the narrow-shape helpers (k_dx_narrow,
// k_head_finish, k_dw_reduce).  Used by the wide train path (B > 512) and by
// forward-only work from 512 rows up.

namespace d4pg {

// ===========================================================================
// MFMA tiled GEMM kernels (wide-batch learner path, f32-in matrix cores)
// ===========================================================================
// For the large-batch config (BASELINE config 5: B=4096, H=1024) the GEMMs
// are compute-bound and belong on the matrix cores.  gfx950's f32-in MFMA
// (v_mfma_f32_32x32x2_f32) runs at the full fp32 rate (157 TF peak) with
// EXACT f32 numerics — bitwise a k-ordered fmaf chain, i.e. the same
// summation order as the per-thread loops of the small-batch kernels.
// Tile: 128x128 per workgroup (4 waves, each 64x64 = 2x2 of 32x32 MFMA
// tiles), K staged through LDS in 32-deep slices.
// M-tile 64 (not 128): the H=1024 layers' grids then cover the chip with
// 2 workgroups per CU, so one workgroup's LDS staging hides behind the
// other's MFMAs (at 128 the 256-wg grid left 1 wg/CU and the per-chunk
// ds_write+barrier was exposed — ~50% MfmaUtil).
#define MT_M 64
#define MT_N 128
#define MT_K 32

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Software-pipelined MFMA tile core of k_mfma_fwd (k_mfma_dx / k_mfma_dw
// carry their own copy of the loop): double-buffered LDS — global loads
// for chunk ch+1 are issued before chunk ch's MFMAs and written to the
// other buffer under them, one barrier per chunk.  `ldA`/`ldB` load chunk
// k0's A/B fragments into the caller's registers, `wr`/`wrs` write them to
// LDS (whole / one slice).
// Staging is VECTORIZED: an all-scalar staging stream (scalar loads +
// per-element bounds checks + scattered ds_writes) was ~350 VALU-pipe
// instructions per chunk — comparable to the chunk's 32 MFMAs' ~1400 MAI
// cycles — capping the H-GEMMs at ~44% of the measured 156 TF/s f32 MFMA
// peak (scripts/mfma_peak, profiles/gemm_lab).  Interior tiles load float4
// and write b128 rows, cutting staging to ~100 instructions; edge tiles
// keep the guarded scalar path with bit-identical LDS contents.
template <typename FA, typename FB, typename FW, typename FWS>
__device__ inline void mfma_pipeline_w(FA ldA, FB ldB, FW wr, FWS wrs,
                                       int nch, float* As0, float* As1,
                                       float* Bs0, float* Bs1, f32x16& a00,
                                       f32x16& a01) {
    int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
    int r = lane & 31, kk2 = lane >> 5;
    ldA(0);
    ldB(0);
    wr(As0, Bs0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        float* As = (ch & 1) ? As1 : As0;
        float* Bs = (ch & 1) ? Bs1 : Bs0;
        float* Asn = (ch & 1) ? As0 : As1;
        float* Bsn = (ch & 1) ? Bs0 : Bs1;
        bool more = ch + 1 < nch;
        if (more) {
            ldA((ch + 1) * MT_K);
            ldB((ch + 1) * MT_K);
        }
        // next chunk's LDS writes ride the MFMA shadows as slices 6..15
        // (slice 6 trails the loads by ~500 MFMA-pipe cycles, past L2
        // latency) instead of bunching at the barrier, where the two
        // co-resident workgroups' bursts convoy and expose the staging
#pragma unroll
        for (int ks = 0; ks < MT_K; ks += 2) {
            float a0 = As[(ks + kk2) * (MT_M + 4) + wm0 + r];
            float b0 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + r];
            float b1 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + 32 + r];
            a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, a00, 0, 0, 0);
            a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, a01, 0, 0, 0);
            if (more) wrs(ks >> 1, Asn, Bsn);
        }
        __syncthreads();
    }
}

#define MFMA_LDS_DECL \
    __shared__ float As2[2][MT_K * (MT_M + 4)]; \
    __shared__ float Bs2[2][MT_K * (MT_N + 4)]

// C[B,out] = act(X[B,in1 (++ concat in2)] @ Wt[in,out] + bias).
// ksplit > 1: split-K over `parts` (disjoint per-segment partials summed
// by k_head_finish) — used for the narrow heads (out <= 64), whose
// M-tile-only grids (64 wgs) otherwise leave 3/4 of the chip idle.
__global__ void __launch_bounds__(256, 2)
k_mfma_fwd(const float* __restrict__ x1, const float* __restrict__ x2,
           const float* __restrict__ wt, const float* __restrict__ bias,
           float* __restrict__ y, int B, int in1, int in2, int out,
           int act_kind, int ksplit, float* __restrict__ parts) {
    MFMA_LDS_DECL;
    int in_total = in1 + in2;
    int ntn = (out + MT_N - 1) / MT_N;
    int ntm = (B + MT_M - 1) / MT_M;
    int seg = blockIdx.x / (ntm * ntn);
    int tile = blockIdx.x % (ntm * ntn);
    int m0 = (tile / ntn) * MT_M, n0 = (tile % ntn) * MT_N;
    int nch_total = (in_total + MT_K - 1) / MT_K;
    int nch_seg = (nch_total + ksplit - 1) / ksplit;
    int ch0 = seg * nch_seg;
    int nch = min(nch_seg, nch_total - ch0);
    int kbase = ch0 * MT_K;
    int tid = threadIdx.x, lane = tid & 63;
    f32x16 acc00 = {}, acc01 = {};
    // vectorized staging geometry (see mfma_pipeline_w):
    //   A: thread owns row m0+tid/4, k-segment (tid%4)*8 -> 2x float4
    //      loads, scalar transposed LDS writes
    //   B: thread owns k-row tid/8, n-segment (tid%8)*16 -> 4x float4
    //      loads AND 4x b128 LDS writes (row-major, no transpose)
    const int am = tid >> 2, ak = (tid & 3) * 8;
    const int bk = tid >> 3, bn = (tid & 7) * 16;
    const bool vecA = (in1 % 4 == 0) && (m0 + MT_M <= B);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= out);
    float ta[8];
    float4 tb[4];
    auto ldA = [&](int k0r) {
        int k0 = kbase + k0r;
        if (vecA && k0 + MT_K <= in1) {
            const float* src = x1 + (long)(m0 + am) * in1 + k0 + ak;
            float4 v0 = *reinterpret_cast<const float4*>(src);
            float4 v1 = *reinterpret_cast<const float4*>(src + 4);
            ta[0] = v0.x; ta[1] = v0.y; ta[2] = v0.z; ta[3] = v0.w;
            ta[4] = v1.x; ta[5] = v1.y; ta[6] = v1.z; ta[7] = v1.w;
        } else {
            int gm = m0 + am;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int gk = k0 + ak + u;
                float v = 0.f;
                if (gm < B && gk < in_total)
                    v = (gk < in1) ? x1[(long)gm * in1 + gk]
                                   : x2[(long)gm * in2 + (gk - in1)];
                ta[u] = v;
            }
        }
    };
    auto ldB = [&](int k0r) {
        int k0 = kbase + k0r;
        int gk = k0 + bk;
        if (vecB && k0 + MT_K <= in_total) {
            const float4* src = reinterpret_cast<const float4*>(
                wt + (long)gk * out + n0 + bn);
#pragma unroll
            for (int u = 0; u < 4; ++u) tb[u] = src[u];
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int gn = n0 + bn + u;
                float v = (gk < in_total && gn < out)
                    ? wt[(long)gk * out + gn] : 0.f;
                reinterpret_cast<float*>(tb)[u] = v;
            }
        }
    };
    auto wr = [&](float* As, float* Bs) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
            As[(ak + u) * (MT_M + 4) + am] = ta[u];
        float4* dst = reinterpret_cast<float4*>(&Bs[bk * (MT_N + 4) + bn]);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[u] = tb[u];
    };
    // sliced form for the in-loop pipeline: A scalar writes at slices
    // 6..13, B b128 writes at 12..15 (two streams overlap harmlessly)
    auto wrs = [&](int sl, float* As, float* Bs) {
        if (sl >= 6 && sl < 14)
            As[(ak + sl - 6) * (MT_M + 4) + am] = ta[sl - 6];
        if (sl >= 12)
            reinterpret_cast<float4*>(
                &Bs[bk * (MT_N + 4) + bn])[sl - 12] = tb[sl - 12];
    };
    mfma_pipeline_w(ldA, ldB, wr, wrs, nch, As2[0], As2[1], Bs2[0], Bs2[1],
                    acc00, acc01);
    int wid = tid >> 6;
    int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
    const f32x16* accs[2] = {&acc00, &acc01};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int i = 0, j = t;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            int col = lane & 31;
            int gm = m0 + wm0 + i * 32 + row;
            int gn = n0 + wn0 + j * 32 + col;
            if (gm < B && gn < out) {
                if (ksplit > 1) {
                    parts[((long)seg * B + gm) * out + gn] =
                        (*accs[t])[reg];
                } else {
                    float v = (*accs[t])[reg] + bias[gn];
                    if (act_kind == ACT_RELU) v = fmaxf(v, 0.f);
                    else if (act_kind == ACT_TANH) v = tanhf(v);
                    y[(long)gm * out + gn] = v;
                }
            }
        }
    }
}

// Narrow dX (span <= 8, the concat action slice): wave per batch row,
// lane-parallel over `out` with shfl reduce.  The MFMA path for this
// shape (one N-tile -> 64-wg grid) left 3/4 of the chip idle and its
// staging fully exposed (~76 us for 50 MFLOP); this VALU form runs the
// whole thing in ~10 us.
__global__ void k_dx_narrow(const float* __restrict__ dz,
                            const float* __restrict__ wt,
                            const float* __restrict__ ymask,
                            float* __restrict__ dx, int B, int in_lo,
                            int in_hi, int out, int prev_act) {
    int lane = threadIdx.x & 63, wrow = threadIdx.x / 64;
    int wpb = blockDim.x / 64;
    int span = in_hi - in_lo;
    for (int row = blockIdx.x * wpb + wrow; row < B;
         row += gridDim.x * wpb) {
        for (int j = 0; j < span; ++j) {
            const float* wrowp = wt + (long)(in_lo + j) * out;
            float acc = 0.f;
            for (int o = lane; o < out; o += 64)
                acc += dz[(long)row * out + o] * wrowp[o];
            for (int s = 32; s > 0; s >>= 1)
                acc += __shfl_xor(acc, s, 64);
            if (lane == 0) {
                float m_ = ymask
                    ? act_mask(prev_act, ymask[(long)row * span + j]) : 1.f;
                dx[(long)row * span + j] = acc * m_;
            }
        }
    }
}

// Head finish: y[row] = act(sum_seg parts[seg][row] + bias), wave == row
// (out <= 64); softmax reduces across the wave (softmax_wave).
__global__ void k_head_finish(const float* __restrict__ parts,
                              const float* __restrict__ bias,
                              float* __restrict__ y, int B, int out,
                              int ksplit, int act_kind) {
    int lane = threadIdx.x & 63, wrow = threadIdx.x / 64;
    int wpb = blockDim.x / 64;
    for (int row = blockIdx.x * wpb + wrow; row < B;
         row += gridDim.x * wpb) {
        float v = 0.f;
        if (lane < out) {
            for (int g = 0; g < ksplit; ++g)
                v += parts[((long)g * B + row) * out + lane];
            v += bias[lane];
        }
        if (act_kind == ACT_SOFTMAX) {
            float sm = softmax_wave(v, lane < out);
            if (lane < out) y[(long)row * out + lane] = sm;
        } else if (lane < out) {
            if (act_kind == ACT_RELU) v = fmaxf(v, 0.f);
            else if (act_kind == ACT_TANH) v = tanhf(v);
            y[(long)row * out + lane] = v;
        }
    }
}

// dX[B, in_lo:in_hi] = (dz[B,out] @ Wt^T) * act'(hprev); hprev/dx are
// [B][span] (span = in_hi - in_lo), hprev null => no mask.
__global__ void __launch_bounds__(256, 2)
k_mfma_dx(const float* __restrict__ dz, const float* __restrict__ wt,
          const float* __restrict__ hprev, float* __restrict__ dx,
          int B, int in_lo, int in_hi, int out, int prev_act) {
    MFMA_LDS_DECL;
    int span = in_hi - in_lo;
    int ntn = (span + MT_N - 1) / MT_N;
    int m0 = (blockIdx.x / ntn) * MT_M;
    int n0 = (blockIdx.x % ntn) * MT_N;             // relative i tile
    int tid = threadIdx.x, lane = tid & 63;
    f32x16 acc00 = {}, acc01 = {};
    // Vectorized staging (see k_mfma_fwd):
    //   A[k(=o)][m(=b)] = dz[b][o]: thread owns dz-row m0+tid/4,
    //     o-segment (tid%4)*8 -> 2x float4 loads, scalar transposed
    //     LDS writes
    //   B[k(=o)][n(=i)] = wt[i][o]: thread owns wt-row in_lo+n0+tid/2,
    //     o-segment (tid%2)*16 -> 4x float4 loads, scalar transposed
    //     LDS writes
    const int am = tid >> 2, ak = (tid & 3) * 8;
    const int bnn = tid >> 1, bkk = (tid & 1) * 16;
    const bool vecA = (out % 4 == 0) && (m0 + MT_M <= B);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= span);
    float ta[8], tb[16];
    auto ldA = [&](int k0) {
        if (vecA && k0 + MT_K <= out) {
            const float* src = dz + (long)(m0 + am) * out + k0 + ak;
            float4 v0 = *reinterpret_cast<const float4*>(src);
            float4 v1 = *reinterpret_cast<const float4*>(src + 4);
            ta[0] = v0.x; ta[1] = v0.y; ta[2] = v0.z; ta[3] = v0.w;
            ta[4] = v1.x; ta[5] = v1.y; ta[6] = v1.z; ta[7] = v1.w;
        } else {
            int gm = m0 + am;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int gk = k0 + ak + u;
                ta[u] = (gm < B && gk < out)
                    ? dz[(long)gm * out + gk] : 0.f;
            }
        }
    };
    auto ldB = [&](int k0) {
        int gi = in_lo + n0 + bnn;
        if (vecB && k0 + MT_K <= out) {
            const float4* src = reinterpret_cast<const float4*>(
                wt + (long)gi * out + k0 + bkk);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                reinterpret_cast<float4*>(tb)[u] = src[u];
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int gk = k0 + bkk + u;
                tb[u] = (gi < in_hi && gk < out)
                    ? wt[(long)gi * out + gk] : 0.f;
            }
        }
    };
    {
        ldA(0);
        ldB(0);
        auto wr = [&](float* As, float* Bs) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                As[(ak + u) * (MT_M + 4) + am] = ta[u];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                Bs[(bkk + u) * (MT_N + 4) + bnn] = tb[u];
        };
        wr(As2[0], Bs2[0]);
        __syncthreads();
        int wid = tid >> 6;
        int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
        int r = lane & 31, kk2 = lane >> 5;
        int nch = (out + MT_K - 1) / MT_K;
        for (int ch = 0; ch < nch; ++ch) {
            float* As = As2[ch & 1];
            float* Bs = Bs2[ch & 1];
            float* Asn = As2[(ch + 1) & 1];
            float* Bsn = Bs2[(ch + 1) & 1];
            bool more = ch + 1 < nch;
            if (more) {
                ldA((ch + 1) * MT_K);
                ldB((ch + 1) * MT_K);
            }
#pragma unroll
            for (int ks = 0; ks < MT_K; ks += 2) {
                float a0 = As[(ks + kk2) * (MT_M + 4) + wm0 + r];
                float b0 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + r];
                float b1 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + 32 + r];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                // next chunk's LDS writes ride the MFMA shadows: one A
                // element + two B elements per slice over slices 6..13
                if (more) {
                    int sl = ks >> 1;
                    if (sl >= 6 && sl < 14) {
                        int u = sl - 6;
                        Asn[(ak + u) * (MT_M + 4) + am] = ta[u];
                        Bsn[(bkk + 2 * u) * (MT_N + 4) + bnn] = tb[2 * u];
                        Bsn[(bkk + 2 * u + 1) * (MT_N + 4) + bnn] =
                            tb[2 * u + 1];
                    }
                }
            }
            __syncthreads();
        }
    }
    int wid = tid >> 6;
    int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
    const f32x16* accs[2] = {&acc00, &acc01};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int i = 0, j = t;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            int col = lane & 31;
            int gm = m0 + wm0 + i * 32 + row;
            int gn = n0 + wn0 + j * 32 + col;          // relative i
            if (gm < B && gn < span) {
                long rel = (long)gm * span + gn;
                float m_ = hprev ? act_mask(prev_act, hprev[rel]) : 1.f;
                dx[rel] = (*accs[t])[reg] * m_;
            }
        }
    }
}

// dWt[in,out] = X^T[in,B] @ dz[B,out]  (K dimension = batch).  Split-K
// over `ksplit` segments (grid = nti*nto*ksplit) with fp32 atomicAdd
// epilogue when ksplit > 1 (dwt/db must be pre-zeroed by the caller in
// that case); bias db[o] = sum_b dz[b][o] accumulates for free out of the
// B-fragment during the MFMA loop (wm0==0 waves of the m0==0 tiles).
// Split-K partial reduce: dwt[i,o] = sum_seg parts[seg][i,o] (+ db tail).
// Replaces the fp32-atomicAdd epilogue of the split-K dW: 2.1M atomics per
// H-layer dW cost ~80 us of L2 read-modify-write serialization, while
// disjoint partials + this bandwidth-bound sweep cost ~3 us
// (profiles/gemm_lab evidence).
__global__ void k_dw_reduce(const float* __restrict__ parts,
                            float* __restrict__ dwt, float* __restrict__ db,
                            long nw, int out, int ksplit) {
    long total = nw + (db ? out : 0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (i < nw) {
            for (int g = 0; g < ksplit; ++g)
                s += parts[(long)g * nw + i];
            dwt[i] = s;
        } else {
            long j = i - nw;
            for (int g = 0; g < ksplit; ++g)
                s += parts[(long)ksplit * nw + (long)g * out + j];
            db[j] = s;
        }
    }
}

__global__ void __launch_bounds__(256, 2)
k_mfma_dw(const float* __restrict__ dz, const float* __restrict__ x1,
          const float* __restrict__ x2, float* __restrict__ dwt,
          float* __restrict__ db, int B, int in1, int in2, int out,
          int ksplit, float* __restrict__ parts) {
    MFMA_LDS_DECL;
    int in_total = in1 + in2;
    int ntn = (out + MT_N - 1) / MT_N;
    int nti = (in_total + MT_M - 1) / MT_M;
    int seg = blockIdx.x / (nti * ntn);
    int tile = blockIdx.x % (nti * ntn);
    int m0 = (tile / ntn) * MT_M;                      // i tile
    int n0 = (tile % ntn) * MT_N;                      // o tile
    int nch_total = (B + MT_K - 1) / MT_K;
    int nch_seg = (nch_total + ksplit - 1) / ksplit;
    int ch0 = seg * nch_seg;
    int nch = min(nch_seg, nch_total - ch0);
    // nch <= 0: an empty tail segment (ceil-split of a batch that is no
    // power-of-two multiple of MT_K, e.g. B=640: 20 chunks over 16
    // segments).  It must still publish ZERO partials — k_dw_reduce sums
    // all ksplit segments, and `parts` holds stale data from earlier GEMMs.
    // All loads below are row-guarded (b_base >= B), the chunk loop is empty.
    long b_base = (long)ch0 * MT_K;
    int tid = threadIdx.x, lane = tid & 63;
    f32x16 acc00 = {}, acc01 = {};
    // Vectorized staging (same rationale as k_mfma_fwd):
    //   A[k(=b)][m(=i)]: thread owns batch-row b_base+k0+tid/8,
    //     i-segment (tid%8)*8 -> 2x float4 loads AND b128 LDS writes
    //     (no transpose: global and LDS are both i-fastest)
    //   B[k(=b)][n(=o)]: thread owns batch-row tid/8, o-segment
    //     (tid%8)*16 -> 4x float4 loads and b128 writes
    const int akb = tid >> 3, ai = (tid & 7) * 8;
    const int bo = (tid & 7) * 16;
    const bool vecA = (in1 % 4 == 0) && (m0 + MT_M <= in1);
    const bool vecB = (out % 4 == 0) && (n0 + MT_N <= out);
    float4 ta[2], tb[4];
    auto ldA = [&](int k0) {
        long gb = b_base + k0 + akb;
        if (vecA && b_base + k0 + MT_K <= B) {
            const float* src = x1 + gb * in1 + m0 + ai;
            ta[0] = *reinterpret_cast<const float4*>(src);
            ta[1] = *reinterpret_cast<const float4*>(src + 4);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int gi = m0 + ai + u;
                float v = 0.f;
                if (gb < B && gi < in_total)
                    v = (gi < in1) ? x1[gb * in1 + gi]
                                   : x2[gb * in2 + (gi - in1)];
                reinterpret_cast<float*>(ta)[u] = v;
            }
        }
    };
    auto ldB = [&](int k0) {
        long gb = b_base + k0 + akb;
        if (vecB && b_base + k0 + MT_K <= B) {
            const float4* src =
                reinterpret_cast<const float4*>(dz + gb * out + n0 + bo);
#pragma unroll
            for (int u = 0; u < 4; ++u) tb[u] = src[u];
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int go = n0 + bo + u;
                reinterpret_cast<float*>(tb)[u] =
                    (gb < B && go < out) ? dz[gb * out + go] : 0.f;
            }
        }
    };
    float bias0 = 0.f, bias1 = 0.f;
    {
        int wid = tid >> 6;
        int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
        int r = lane & 31, kk2 = lane >> 5;
        ldA(0);
        ldB(0);
        auto wr = [&](float* As, float* Bs) {
            float4* da =
                reinterpret_cast<float4*>(&As[akb * (MT_M + 4) + ai]);
            da[0] = ta[0];
            da[1] = ta[1];
            float4* dbp =
                reinterpret_cast<float4*>(&Bs[akb * (MT_N + 4) + bo]);
#pragma unroll
            for (int u = 0; u < 4; ++u) dbp[u] = tb[u];
        };
        wr(As2[0], Bs2[0]);
        __syncthreads();
        for (int ch = 0; ch < nch; ++ch) {
            float* As = As2[ch & 1];
            float* Bs = Bs2[ch & 1];
            float* Asn = As2[(ch + 1) & 1];
            float* Bsn = Bs2[(ch + 1) & 1];
            bool more = ch + 1 < nch;
            if (more) {
                ldA((ch + 1) * MT_K);
                ldB((ch + 1) * MT_K);
            }
#pragma unroll
            for (int ks = 0; ks < MT_K; ks += 2) {
                float a0 = As[(ks + kk2) * (MT_M + 4) + wm0 + r];
                float b0 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + r];
                float b1 = Bs[(ks + kk2) * (MT_N + 4) + wn0 + 32 + r];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                if (wm0 == 0) { bias0 += b0; bias1 += b1; }
                // next chunk's LDS writes ride the MFMA shadows
                if (more) {
                    int sl = ks >> 1;
                    if (sl == 6)
                        reinterpret_cast<float4*>(
                            &Asn[akb * (MT_M + 4) + ai])[0] = ta[0];
                    else if (sl == 7)
                        reinterpret_cast<float4*>(
                            &Asn[akb * (MT_M + 4) + ai])[1] = ta[1];
                    else if (sl >= 8 && sl < 12)
                        reinterpret_cast<float4*>(
                            &Bsn[akb * (MT_N + 4) + bo])[sl - 8] = tb[sl - 8];
                }
            }
            __syncthreads();
        }
    }
    int wid = tid >> 6;
    int wm0 = (wid >> 1) * 32, wn0 = (wid & 1) * 64;
    const f32x16* accs[2] = {&acc00, &acc01};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int i = 0, j = t;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            int col = lane & 31;
            int gi = m0 + wm0 + i * 32 + row;
            int go = n0 + wn0 + j * 32 + col;
            if (gi < in_total && go < out) {
                if (ksplit > 1)
                    // disjoint per-segment partials (k_dw_reduce sums)
                    parts[((long)seg * in_total + gi) * out + go] =
                        (*accs[t])[reg];
                else
                    dwt[(long)gi * out + go] = (*accs[t])[reg];
            }
        }
    }
    if (db && wm0 == 0 && m0 == 0) {
        // combine the two k-parity halves (lane l and l^32 share a column)
        bias0 += __shfl_xor(bias0, 32, 64);
        bias1 += __shfl_xor(bias1, 32, 64);
        int r = lane & 31;
        if ((lane >> 5) == 0) {
            int go0 = n0 + wn0 + r, go1 = n0 + wn0 + 32 + r;
            if (ksplit > 1) {
                long off = (long)ksplit * in_total * out + (long)seg * out;
                if (go0 < out) parts[off + go0] = bias0;
                if (go1 < out) parts[off + go1] = bias1;
            } else {
                if (go0 < out) db[go0] = bias0;
                if (go1 < out) db[go1] = bias1;
            }
        }
    }
}

}  // namespace d4pg
