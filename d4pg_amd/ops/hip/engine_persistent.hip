// Persistent whole-step megakernel k_step_persistent and its p_* phase helpers.
// Used by whole train steps at B <= 256, the flagship regime: ONE kernel runs
// the step (and an nsteps loop of steps) as layer-parallel phases over PNWG =
// 96 co-resident workgroups separated by a software grid barrier (tree
// arrival + write-once go-flag): 7 grid barriers per steady-state step at
// B <= 64, 12 on a launch's first step.  Each GEMM/dX phase tiles 4 rows x 64
// cols per workgroup with register-batched, double-buffered LDS staging; at
// B <= 64 the PER write-back, the next step's sampling and its critic forward
// hide beside the row-local quad chains (elsewhere under the dW/Adam phases).
// At B=64 the step is latency-bound (PMC: 3% VALUBusy), so the design
// maximizes memory-level parallelism, not FLOPs.
//
// HAND-OFF RULE.  Inside a phase, workgroups pass data through q_bar / t_bar,
// which carry NO cache fence: every store another workgroup reads before the
// phase's closing p_bar is a write-through st_wt(), and every load of bytes
// another workgroup wrote inside the current phase is an ld_wt() into
// registers.  A new load of in-phase data must be an ld_wt() load.  Only
// p_bar, the grid barrier, writes L2 back and invalidates L1.

namespace d4pg {

// ===========================================================================
// Persistent whole-step megakernel (flagship small-batch learner path)
// ===========================================================================
// Rationale (measured, profiles/step_kernel_stats round 1): the row-block
// path spends 451 of 497 us/step in two kernels where each of B=64 waves
// re-streams EVERY layer weight from L2 with only 16 workgroups in flight —
// 64x redundant weight traffic and no latency hiding.  This kernel instead
// runs the WHOLE train step (PER sample -> forwards -> C51 projection ->
// CE/policy grads -> dX/dW backward -> Adam+soft-update -> PER write-back)
// as ONE persistent kernel: PNWG=96 workgroups x 256 threads (guaranteed
// co-resident on 256 CUs, so a software grid barrier is deadlock-free),
// layer-parallel phases separated by grid barriers.  Each phase tiles
// its GEMM over the grid (4-row x 64-col tiles, x rows staged in LDS,
// weight columns read once per row-tile instead of once per row), so
// weight traffic drops ~4x and every phase has 16-64 workgroups of
// parallelism.  nsteps loop inside the kernel => zero host involvement
// between steps (the hipGraph path is only needed for the wide-batch
// configs that use the per-layer kernels above).
#define PNWG 96
// derived persistent-grid split points (fractions of PNWG)
#define PW4 (PNWG / 4)
#define PW3A (PNWG / 3)
#define PW3B (PNWG - 2 * (PNWG / 3))
// 4-row x 64-col tiles: a 64x256x256 GEMM phase becomes 64 tiles — the
// whole grid — with ~1 us of FMA per tile (16-row tiles measured ~6 us of
// per-wave compute and left 48 workgroups idle; scripts/tile_bench.hip)
#define PROWS 4
#define PXMAX 512
#define PWOFF (PROWS * PXMAX)
// LDS pool, 12864 floats.  The largest user is p_dw2 (two [64][68] slices =
// 8704 floats); p_fwd / p_bwd_dx need PWOFF + 64 * 68 = 6400.  The other
// 4160 floats are slack: nothing uses them, and shrinking the pool would
// change the kernel's LDS footprint (52,480 B with per_write_leaves' smax).
#define PLDS_FLOATS (2 * 4 * PXMAX + 2 * 64 * 68 + 64)

// phase timing probe: wg0/lane0 stamps the wall clock (100 MHz constant
// clock) after each barrier of ONE step of a launch; read back via
// read_buffer("tstamp") to locate slow phases.  The stamped step is `pts`
// (k_step_persistent: step 1 of a multi-step launch, the first that runs
// the pipelined steady-state schedule; step 0 of a one-step launch).
// PTIMEW stamps from workgroup w instead (the crews' end stamps, slots
// 52-55).
#define PTIMEW(g, s, i, w) \
    do { if ((int)blockIdx.x == (w) && threadIdx.x == 0 && (s) == pts) \
        (g).tstamp[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PTIME(g, s, i) PTIMEW(g, s, i, 0)

// Only p_bar, the grid barrier, still fences, and its two fences are
// one-directional: the release before the arrival writes this workgroup's
// stores back, the acquire after the wait drops the CU's stale L1 lines.
// (__threadfence() does both; two of them per barrier cost the flagship
// step ~19 us — 4616 -> 5041 steps/s, NOTES.md.)  The explicit vmcnt wait
// keeps the arrival, and the loads after the barrier, behind the fence's
// own wait.  q_bar and t_bar carry no fence at all: what crosses them
// follows the hand-off rule in the file header (st_wt / ld_wt below).
__device__ inline void bar_release() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ inline void bar_acquire() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

typedef __attribute__((address_space(1))) unsigned long long gu64;

// Fence-free arrival + wait of q_bar / t_bar: every wave drains its own
// write-through stores, the workgroup barrier collects the waves, one lane
// adds to the group's counter and polls it with L1-bypassing loads.  The
// wavefront-scope fence emits no instruction; it keeps the compiler from
// hoisting loads above the poll.  Bounded spin as in p_bar.
__device__ __forceinline__ void bar_handoff(unsigned long long* ctr,
                                            unsigned long long want) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(ctr, 1ull);
        long spins = 0;
        while (__hip_atomic_load((gu64*)ctr, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) < want) {
            if (++spins > (1L << 26)) break;
            __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
}

// software grid barrier — tree arrival + write-once go-flag.  Safe because
// all PNWG workgroups are co-resident (256 wgs of 256 threads, one per CU
// — validated by the ctor's occupancy gate).
//
// Layout in gbar[]: 8 group counters at [g*16] (separate 128 B lines),
// root counter at [128], go-flag at [144], cross-launch round base at
// [160] (written by wg 0 after the final barrier; stream order makes the
// next launch's read race-free).
//
// Design notes (measured): a single central atomic that everyone arrives
// on AND polls makes idle workgroups' poll storm contend with the active
// workgroups' real memory traffic — single-GEMM phases went from ~6 us to
// ~40 us under it.  Here arrivals fan in through per-group lines, pollers
// read only the once-written flag, and the spin backs off exponentially
// (s_sleep needs an immediate, hence the two-stage backoff).
__device__ inline void p_bar(unsigned long long* gb,
                             unsigned long long& round) {
    __syncthreads();
    round += 1;
    if (threadIdx.x == 0) {
        bar_release();                         // flush our writes
        int grp = blockIdx.x & 7;
        unsigned long long old = atomicAdd(&gb[grp << 4], 1ull);
        if (old + 1 == round * (PNWG >> 3)) {  // last of the group
            unsigned long long r = atomicAdd(&gb[128], 1ull);
            if (r + 1 == round * 8)            // last group overall
                __hip_atomic_store(&gb[144], round, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        volatile unsigned long long* f = &gb[144];
        volatile unsigned long long* err = &gb[176];  // timeout flag (own line)
        long spins = 0;
        while (*f < round) {
            // safety valve: a barrier logic bug (or non-co-resident grid)
            // must never hard-hang the GPU.  On timeout (~10 s) raise the
            // error flag and bail; other workgroups see the flag on their
            // next poll-check and drain out instead of each spinning the
            // full 10 s.  The host checks the flag after every step() /
            // sync and throws — the step's results are NOT used.
            if (++spins > (1L << 26)) {
                atomicAdd((unsigned long long*)err, 1ull);
                break;
            }
            // barriers resolve in ~2-5 us: stay on the fast poll long
            // enough to catch that window before backing off.  The error
            // check rides the slow path only (every 64th backoff poll, to
            // keep poll traffic off the shared error line).
            if (spins < 48) __builtin_amdgcn_s_sleep(2);
            else {
                __builtin_amdgcn_s_sleep(32);
                if ((spins & 63) == 0 && *err) break;
            }
        }
        bar_acquire();                         // invalidate L1
    }
    __syncthreads();
}

// quad-local barrier: synchronizes the 4 workgroups of one quad (a
// row-group's column-tile team in the chained fwd/bwd blocks) without
// touching the grid barrier.  Each quad owns its own 128 B line at
// gbar[192 + q*16]; arrivals and polls stay quad-private, so 16 quads
// proceed fully independently (~0.5-1 us vs ~3.3 us for the grid form).
// qround carries across launches like the grid round: members read the
// line once at kernel entry (ordered before any arrival by the first
// grid barrier) and count from there.  No fence: see bar_handoff.
__device__ inline void q_bar(unsigned long long* qc,
                             unsigned long long& qround) {
    qround += 4;
    bar_handoff(qc, qround);
}
// (A per-member slot-store variant — release stores + one-line relaxed
// polls instead of the shared atomic counter — measured SLOWER: 3674 vs
// 3773 steps/s; the four poll loads don't coalesce into one L2 access.)

// group barrier for the policy-block tail crew (q_bar with a caller-set
// member count; own line at gbar[1280])
__device__ inline void t_bar(unsigned long long* tc,
                             unsigned long long& trnd, int members) {
    trnd += members;
    bar_handoff(tc, trnd);
}

// Tiled forward: 4-row x 64-col tiles, one row per wave; x rows staged in
// LDS (broadcast reads), weight column read ONCE per tile (not once per
// row).  Thread (rq = tid/64, c = tid%64) accumulates row r0+rq of column
// c0+c; softmax (out<=64) reduces per-row across the wave.  Summation order
// over k is ascending, matching the eager/rowblock paths bit-for-bit.
// x1 / x2 may have been written by another workgroup inside this phase and
// y may be read by one: ld_wt loads, st_wt stores, whoever calls (the
// hand-off rule).  Weights and biases were published behind a p_bar.
// (__noinline__ is load-bearing: inlining 15 copies into the persistent
// kernel segfaults ROCm 7.2's clang in ADCE; the call overhead is noise
// next to the ~1 us phase time.)
// TWIN: each instantiation of k_step_persistent calls its own copy of the two
// out-of-line helpers (p_fwd, p_dw2), the code being the same (TWIN numbers
// the instantiation: CLIP + 2 * QR).  An
// out-of-line function shared by two kernels changes the register allocation
// of both (measured: the default kernel went from 598 to 658 spilled SGPRs
// and from 84 to 216 B of scratch); with a copy each, the default kernel
// compiles to exactly what it was before the clip-on one existed.
template <int TWIN>
__device__ __noinline__ void p_fwd(float* lds, const float* x1, const float* x2,
                             const float* wt, const float* bias, float* y,
                             int B, int in1, int in2, int out, int act_kind,
                             int wg_rel, int nwg) {
    int in_total = in1 + in2;
    // x rows staged at a 4-float-aligned stride so the k-loop can read
    // them with ds_read_b128 (16 B alignment)
    int in_pad = (in_total + 3) & ~3;
    int nrt = (B + PROWS - 1) / PROWS;
    int nct = (out + 63) / 64;
    int ntiles = nrt * nct;
    int tid = threadIdx.x;
    for (int t = wg_rel; t < ntiles; t += nwg) {
        int r0 = (t / nct) * PROWS, c0 = (t % nct) * 64;
        int kk16 = tid >> 6, cc16 = tid & 63;
        float wreg[16];
        int nfull = in_total >> 6;
        auto preload = [&](int kc) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int gk = kc + kk16 + 4 * u, gc = c0 + cc16;
                wreg[u] = (gc < out)
                    ? wt[(long)gk * out + gc] : 0.f;
            }
        };
        // first weight chunk's loads fly WITH the x-stage loads (the
        // x ds_writes only wait on the older x loads)
        if (nfull > 0) preload(0);
        // x-stage, register-batched (all loads in flight, then ds_writes)
        {
            int tot = PROWS * in_pad;
            for (int base = 0; base < tot; base += 256 * 8) {
                float tmp[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int e = base + u * 256 + tid;
                    float v = 0.f;
                    if (e < tot) {
                        int rr_ = e / in_pad, kk = e % in_pad;
                        int gb = r0 + rr_;
                        if (gb < B && kk < in_total)
                            v = (kk < in1)
                                ? ld_wt(&x1[(long)gb * in1 + kk])
                                : ld_wt(&x2[(long)gb * in2 + (kk - in1)]);
                    }
                    tmp[u] = v;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int e = base + u * 256 + tid;
                    if (e < tot) lds[e] = tmp[u];
                }
            }
        }
        __syncthreads();
        int rq = tid >> 6, c = tid & 63;
        int o = c0 + c;
        int r = r0 + rq;
        float acc = 0.f;
        // weight slice K-chunked through LDS in [col][k] layout (row
        // stride 68 floats: 16 B-aligned and 4-bank-strided across
        // lanes), so the k-loop fetches 4 k at a time with ONE
        // ds_read_b128 per operand — the b32 form issued 3 LDS reads
        // per k and was issue-bound, not bandwidth-bound.  Summation
        // stays ascending-k: bitwise identical to the eager oracle.
        float* ws = lds + PWOFF;                 // [64 cols][68 k]
        const float* xr = lds + rq * in_pad;
        for (int ch = 0; ch < nfull; ++ch) {
            int kc = ch << 6;
            float wb[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wb[u] = wreg[u];
            if (kc + 64 < (nfull << 6)) preload(kc + 64);
#pragma unroll
            for (int u = 0; u < 16; ++u)
                ws[cc16 * 68 + kk16 + 4 * u] = wb[u];
            __syncthreads();
            if (o < out) {
                const float* wcol = ws + c * 68;
#pragma unroll
                for (int k = 0; k < 64; k += 4) {
                    float4 wv = *reinterpret_cast<const float4*>(wcol + k);
                    float4 xv = *reinterpret_cast<const float4*>(
                        xr + kc + k);
                    acc += xv.x * wv.x;
                    acc += xv.y * wv.y;
                    acc += xv.z * wv.z;
                    acc += xv.w * wv.w;
                }
            }
            __syncthreads();
        }
        int kc = nfull << 6, klen = in_total - kc;
        if (klen > 0) {
            for (int e = tid; e < (klen << 6); e += 256) {
                int kk = e >> 6, cc = e & 63;
                int gc = c0 + cc;
                ws[cc * 68 + kk] = (gc < out)
                    ? wt[(long)(kc + kk) * out + gc] : 0.f;
            }
            __syncthreads();
            if (o < out) {
                for (int k = 0; k < klen; ++k)
                    acc += xr[kc + k] * ws[c * 68 + k];
            }
            __syncthreads();
        }
        if (act_kind == ACT_SOFTMAX) {
            // out <= 64, single col-chunk; wave == one row.  This is
            // softmax_wave written out: calling the helper here changes
            // p_fwd's code enough to cost the flagship step 0.8% (measured,
            // 4,255 vs 4,288 steps/s), with equal results.
            float v = (o < out) ? acc + bias[o] : -INFINITY;
            float mx = v;
            for (int s = 32; s > 0; s >>= 1)
                mx = fmaxf(mx, __shfl_xor(mx, s, 64));
            float e = (o < out) ? __expf(v - mx) : 0.f;
            float sum = e;
            for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
            if (r < B && o < out) st_wt(&y[(long)r * out + o], e / sum);
        } else if (r < B && o < out) {
            float v = acc + bias[o];
            if (act_kind == ACT_RELU) v = fmaxf(v, 0.f);
            else if (act_kind == ACT_TANH) v = tanhf(v);
            st_wt(&y[(long)r * out + o], v);
        }
        __syncthreads();
    }
}

// Tiled backward-dX: dx[b][i-in_lo] = (sum_o dz[b][o] wt[i][o]) * mask.
// dz rows staged in LDS; mask/dx arrays are [B][span] (span = in_hi-in_lo):
// full-range h arrays and the concat action slice both fit this form.
// dz and hprev are ld_wt loads and dx an st_wt store (the hand-off rule).
__device__ inline void p_bwd_dx(float* lds, const float* dz, const float* wt,
                                int in_lo, int in_hi, int out, int B,
                                const float* hprev, int prev_act, float* dx,
                                int wg_rel, int nwg) {
    int span = in_hi - in_lo;
    int nrt = (B + PROWS - 1) / PROWS;
    int nit = (span + 63) / 64;
    int ntiles = nrt * nit;
    int tid = threadIdx.x;
    for (int t = wg_rel; t < ntiles; t += nwg) {
        int r0 = (t / nit) * PROWS, i0 = in_lo + (t % nit) * 64;
        int oo16 = tid & 3;
        int ii16 = tid >> 2;
        float wreg[16];
        int gi_ld = i0 + ii16;
        int nfull = out >> 6;
        auto preload = [&](int oc) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int go = oc + oo16 + 4 * u;
                wreg[u] = (gi_ld < in_hi)
                    ? wt[(long)gi_ld * out + go] : 0.f;
            }
        };
        if (nfull > 0) preload(0);
        // dz-stage, register-batched; rows padded to 4-float stride so
        // the o-loop reads them with ds_read_b128
        int out_pad = (out + 3) & ~3;
        {
            int tot = PROWS * out_pad;
            for (int base = 0; base < tot; base += 256 * 8) {
                float tmp[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int e = base + u * 256 + tid;
                    float v = 0.f;
                    if (e < tot) {
                        int rr_ = e / out_pad, oo = e % out_pad;
                        int gb = r0 + rr_;
                        if (gb < B && oo < out)
                            v = ld_wt(&dz[(long)gb * out + oo]);
                    }
                    tmp[u] = v;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int e = base + u * 256 + tid;
                    if (e < tot) lds[e] = tmp[u];
                }
            }
        }
        __syncthreads();
        int rq = tid >> 6, c = tid & 63;
        int i = i0 + c;
        int r = r0 + rq;
        float acc = 0.f;
        // weight tile O-chunked through LDS in [i][o] layout (stride 68:
        // 16 B-aligned rows), so the o-loop fetches 4 o per ds_read_b128
        // for both operands — see p_fwd's identical rework; summation
        // stays ascending-o, bitwise identical
        float* ws = lds + PWOFF;                 // [64 i][68 o]
        const float* zr = lds + rq * out_pad;
        for (int ch = 0; ch < nfull; ++ch) {
            int oc = ch << 6;
            float wb[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wb[u] = wreg[u];
            if (oc + 64 < (nfull << 6)) preload(oc + 64);
#pragma unroll
            for (int u = 0; u < 16; ++u)
                ws[ii16 * 68 + oo16 + 4 * u] = wb[u];
            __syncthreads();
            if (i < in_hi) {
                const float* wrow = ws + c * 68;
#pragma unroll
                for (int o = 0; o < 64; o += 4) {
                    float4 wv = *reinterpret_cast<const float4*>(wrow + o);
                    float4 zv = *reinterpret_cast<const float4*>(
                        zr + oc + o);
                    acc += zv.x * wv.x;
                    acc += zv.y * wv.y;
                    acc += zv.z * wv.z;
                    acc += zv.w * wv.w;
                }
            }
            __syncthreads();
        }
        int oc = nfull << 6, olen = out - oc;
        if (olen > 0) {
            for (int e = tid; e < 4096; e += 256) {
                int ii = e >> 6, oo = e & 63;
                int gi = i0 + ii;
                ws[ii * 68 + oo] = (gi < in_hi && oo < olen)
                    ? wt[(long)gi * out + (oc + oo)] : 0.f;
            }
            __syncthreads();
            if (i < in_hi) {
                for (int o = 0; o < olen; ++o)
                    acc += zr[oc + o] * ws[c * 68 + o];
            }
            __syncthreads();
        }
        if (r < B && i < in_hi) {
            long rel = (long)r * span + (i - in_lo);
            float m_ = hprev ? act_mask(prev_act, ld_wt(&hprev[rel])) : 1.f;
            st_wt(&dx[rel], acc * m_);
        }
        __syncthreads();
    }
}

// dW tile [64 i x 64 o] per wg: x^T and dz chunks staged in LDS (coalesced),
// each thread owns a 4x4 output patch (ig = tid>>4 picks 4 i's, og = tid&15
// picks 4 o's) — 8 LDS reads + 16 FMAs per batch row.  Bias rows fold in on
// the i0==0 tiles.  Accumulation over b is ascending.
template <int TWIN>                   // see p_fwd
__device__ __noinline__ void p_dw2(float* lds, const float* dz,
                                   const float* x1, const float* x2,
                                   float* dwt, float* dbias,
                                   int B, int in1, int in2, int out,
                                   int wg_rel, int nwg) {
    int in_total = in1 + in2;
    int nti = (in_total + 63) >> 6, nto = (out + 63) >> 6;
    int ntiles = nti * nto;
    float* xs = lds;                       // [64 b][68] i-slice
    float* zs = lds + 64 * 68;             // [64 b][68] o-slice
    // row stride 68: 16 B-aligned so the b-loop reads each 4-wide
    // register block with ONE ds_read_b128 (see p_fwd's rework)
    int tid = threadIdx.x;
    int ig = tid >> 4, og = tid & 15;
    for (int t = wg_rel; t < ntiles; t += nwg) {
        int i0 = (t / nto) << 6, o0 = (t % nto) << 6;
        float acc[4][4] = {};
        float accb[4] = {};
        for (int bc = 0; bc < B; bc += 64) {
            // register-batched staging (all 32 loads in flight)
            float tx[16], tz[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int e = u * 256 + tid;
                int bb = e >> 6, ii = e & 63;
                int gb = bc + bb, gi = i0 + ii;
                float xv = 0.f;
                if (gb < B && gi < in_total)
                    xv = (gi < in1) ? x1[(long)gb * in1 + gi]
                                    : x2[(long)gb * in2 + (gi - in1)];
                tx[u] = xv;
                int go = o0 + ii;
                tz[u] = (gb < B && go < out)
                    ? dz[(long)gb * out + go] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                int e = u * 256 + tid;
                int bb = e >> 6, ii = e & 63;
                xs[bb * 68 + ii] = tx[u];
                zs[bb * 68 + ii] = tz[u];
            }
            __syncthreads();
            int blim = min(64, B - bc);
            for (int b = 0; b < blim; ++b) {
                float4 xq = *reinterpret_cast<const float4*>(
                    xs + b * 68 + ig * 4);
                float4 zq = *reinterpret_cast<const float4*>(
                    zs + b * 68 + og * 4);
                float xv0 = xq.x, xv1 = xq.y, xv2 = xq.z, xv3 = xq.w;
                float zv0 = zq.x, zv1 = zq.y, zv2 = zq.z, zv3 = zq.w;
                acc[0][0] += xv0 * zv0; acc[0][1] += xv0 * zv1;
                acc[0][2] += xv0 * zv2; acc[0][3] += xv0 * zv3;
                acc[1][0] += xv1 * zv0; acc[1][1] += xv1 * zv1;
                acc[1][2] += xv1 * zv2; acc[1][3] += xv1 * zv3;
                acc[2][0] += xv2 * zv0; acc[2][1] += xv2 * zv1;
                acc[2][2] += xv2 * zv2; acc[2][3] += xv2 * zv3;
                acc[3][0] += xv3 * zv0; acc[3][1] += xv3 * zv1;
                acc[3][2] += xv3 * zv2; acc[3][3] += xv3 * zv3;
                if (ig == 0 && i0 == 0) {
                    accb[0] += zv0; accb[1] += zv1;
                    accb[2] += zv2; accb[3] += zv3;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int gi = i0 + ig * 4 + a;
            if (gi >= in_total) continue;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                int go = o0 + og * 4 + bb;
                if (go < out) dwt[(long)gi * out + go] = acc[a][bb];
            }
        }
        if (ig == 0 && i0 == 0 && dbias) {
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                int go = o0 + og * 4 + bb;
                if (go < out) dbias[go] = accb[bb];
            }
        }
    }
}

// CLIP: the gradient enters as scale * gr[i], rounded once before the update
// reads it, as in k_adam_lerp_clip; the slab keeps the raw gradient.
template <bool CLIP>
__device__ inline void p_adam_lerp(float* __restrict__ p,
                                   const float* __restrict__ gr,
                                   float* __restrict__ m,
                                   float* __restrict__ v,
                                   float* __restrict__ tgt_slab, long n,
                                   float lr, float tau, long long t,
                                   float scale, int nwg = PNWG) {
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    AdamBias bc = adam_bias(b1, b2, t);
    // register-batched: fire all 5 streams' loads for 4 grid-strides at
    // once (a serial load->compute->store loop pays one memory round-trip
    // per element batch)
    long stride = (long)nwg * 256;
    long i0 = (long)blockIdx.x * 256 + threadIdx.x;
    for (long base = i0; base < n; base += stride * 4) {
        float gi_[4], mi_[4], vi_[4], pi_[4], ti_[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            long i = base + u * stride;
            bool ok = i < n;
            gi_[u] = ok ? gr[i] : 0.f;
            mi_[u] = ok ? m[i] : 0.f;
            vi_[u] = ok ? v[i] : 0.f;
            pi_[u] = ok ? p[i] : 0.f;
            ti_[u] = ok ? tgt_slab[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            long i = base + u * stride;
            if (i >= n) continue;
            // k_adam_lerp's element update, written out in both (see
            // adam_bias for why it is not one helper)
            float gi = CLIP ? __fmul_rn(scale, gi_[u]) : gi_[u];
            float mi = b1 * mi_[u] + (1.f - b1) * gi;
            float vi = b2 * vi_[u] + (1.f - b2) * gi * gi;
            m[i] = mi; v[i] = vi;
            float pn = pi_[u] - lr * (mi / bc.bc1)
                                   / (sqrtf(vi / bc.bc2) + eps);
            p[i] = pn;
            tgt_slab[i] = ti_[u] + tau * (pn - ti_[u]);
        }
    }
}

// Gradient-clip phase of the clip-on kernel: the workgroups take the slab's
// GN_CHUNK chunks round-robin and write their double sums of squares to
// gn_part.  The caller's p_bar publishes them (they cross a grid barrier:
// plain stores and loads, the hand-off rule); after it every workgroup that
// runs Adam sums the partials itself (p_grad_scale), so no broadcast is needed.
__device__ inline void p_grad_sumsq(const float* gr, long n, double* gn_part,
                                    float* lds) {
    double* red = reinterpret_cast<double*>(lds);
    int nc = gn_chunks(n);
    for (int c = (int)blockIdx.x; c < nc; c += PNWG)
        grad_sumsq_chunk(gr, n, c, gn_part, red);
}

// ... and the scale from the published partials; workgroup 0 records it.
__device__ inline float p_grad_scale(const StepArgs& g, int is_actor) {
    GradClip c = grad_clip_finish(is_actor ? g.gn_part_a : g.gn_part_c,
                                  is_actor ? g.n_actor : g.n_critic,
                                  g.max_grad_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        grad_stats_write(g.gstat, is_actor, c);
    return c.scale;
}

// sample + gather phase, PER or uniform (one wave per probe, like
// k_per_sample)
__device__ inline void p_sample(const StepArgs& g, int wg0,
                                long long epoch, long long beta_t,
                                float* bs_out) {
    // wg0: first workgroup of the sampling crew.  epoch / beta_t: the
    // schedule values of the step being sampled (k_step_persistent reads
    // the counters ONCE per launch and threads base+s through, so the
    // NEXT step's batch can be pre-sampled before the counters advance).
    // bs_out: which state buffer to gather into (double-buffered by step
    // parity).
    int probe = ((int)blockIdx.x - wg0) * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (probe >= g.B) return;
    sample_probe<true>(g, bs_out, probe, lane, epoch, beta_t);
}

// merged projection + CE-grad phase: the wave that projects row b's target
// distribution keeps it in LDS and computes the CE gradient/priority
// immediately (saves a barrier and the m_proj global round-trip; q comes
// from PH4).  m_proj is still written out for introspection/parity tests.
// QR (the quantile head): p_t holds theta', the same wave writes the target
// samples T to its LDS row and to m_proj and takes the quantile-Huber
// gradient, row loss and priority from them; same loads and stores otherwise.
template <bool QR>
__device__ inline void p_project_ce(const StepArgs& g, float* lds,
                                    int row_base = -1) {
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int row = (row_base < 0 ? (int)blockIdx.x * 4 : row_base) + wid;
    if (row >= g.B) return;
    int K = g.K;
    float* mrow = lds + wid * 64;
    if (QR) {
        float tp = (lane < K) ? ld_wt(&g.p_t[(long)row * K + lane]) : 0.f;
        float t = qr_target_row(mrow, tp, g.br[row], g.bd[row], g.gamma_n, K,
                                lane);
        float th = 0.f;
        if (lane < K) {
            g.m_proj[(long)row * K + lane] = t;
            th = g.q[(long)row * K + lane];
        }
        float scale = (g.is_weighting && g.bw) ? g.bw[row] : 1.f;
        QrRow r = qr_grad_row(mrow, th, scale, g.B, K, g.kappa, g.per_eps,
                              lane);
        if (lane < K) g.dlog[(long)row * K + lane] = r.dz;
        if (lane == 0) {
            g.pri[row] = r.pri;
            atomicAdd(&g.cnt->loss_critic, scale * r.loss / (float)g.B);
        }
        return;
    }
    // p_t: this workgroup's own st_wt store of a moment ago (K <= 64 is one
    // column tile, member 0's); ld_wt so that no older L1 line can serve it.
    // q, br, bd, bw and the stores below cross a p_bar: plain.
    float p = (lane < K) ? ld_wt(&g.p_t[(long)row * K + lane]) : 0.f;
    c51_project_row(mrow, p, g.br[row], g.bd[row], g.v_min, g.v_max,
                    g.gamma_n, K, lane);
    float qv = 0.f, mv = 0.f;
    if (lane < K) {
        g.m_proj[(long)row * K + lane] = mrow[lane];
        qv = g.q[(long)row * K + lane];
        mv = mrow[lane];
    }
    float scale = (g.is_weighting && g.bw) ? g.bw[row] : 1.f;
    CeRow r = ce_grad_row(mv, qv, scale, g.B);
    if (lane < K) g.dlog[(long)row * K + lane] = r.dz;
    float pri = ce_priority_row(mv, qv, r.dot,
                                c51_atom(g.v_min, g.v_max, K, lane),
                                g.true_td, g.per_eps);
    if (lane == 0) {
        g.pri[row] = pri;
        atomicAdd(&g.cnt->loss_critic, scale * r.ce / (float)g.B);
    }
}

// narrow backward-dX (span <= 8, e.g. the concat action slice): one wave
// per batch row, lane-parallel dot over `out` with a shfl reduce, tanh
// mask applied from ymask.  dz and ymask are handed off in-phase (ld_wt),
// dx is read by the next layer's quad (st_wt).
__device__ inline void p_bwd_dx_narrow(const StepArgs& g, const float* dz,
                                       const float* wt, int in_lo,
                                       int in_hi, int out,
                                       const float* ymask, float* dx,
                                       int row_base = -1) {
    int row = (row_base < 0 ? (int)blockIdx.x * 4 : row_base)
              + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (row >= g.B) return;
    int span = in_hi - in_lo;
    for (int j = 0; j < span; ++j) {
        const float* wrow = wt + (long)(in_lo + j) * out;
        float acc = 0.f;
        for (int o = lane; o < out; o += 64)
            acc += ld_wt(&dz[(long)row * out + o]) * wrow[o];
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (lane == 0) {
            float y = ld_wt(&ymask[(long)row * span + j]);
            st_wt(&dx[(long)row * span + j], acc * (1.f - y * y));
        }
    }
}

template <bool QR>
__device__ inline void p_policy_grad(const StepArgs& g,
                                     int row_base = -1) {
    int row = (row_base < 0 ? (int)blockIdx.x * 4 : row_base)
              + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (row >= g.B) return;
    int K = g.K;
    // pq: K <= 64 (step_path's gate) makes pc.L4 ONE column tile, member
    // 0's, and member 0 alone calls this: the rows read here are this
    // workgroup's own st_wt stores, no other workgroup's.  ld_wt all the
    // same, so that no older L1 line can serve them.
    float qv = (lane < K) ? ld_wt(&g.pq[(long)row * K + lane]) : 0.f;
    float e;
    float dz = QR ? qr_policy_row(qv, g.B, K, lane, e)
                  : policy_grad_row(qv, c51_atom(g.v_min, g.v_max, K, lane),
                                    g.B, e);
    if (lane < K) st_wt(&g.pd3[(long)row * K + lane], dz);
    if (lane == 0) atomicAdd(&g.cnt->loss_actor, -e / (float)g.B);
}

// PER write-back (k_per_update without its counter tick — k_step_persistent
// advances the counters once per launch); one workgroup, `owner_wg`, does it
__device__ inline void p_per_update(const StepArgs& g, int owner_wg) {
    // uniform replay has no trees: skip the work, never a barrier arrival
    // (the callers' t_bar / p_bar stay where they are)
    if ((int)blockIdx.x != owner_wg || !g.prioritized) return;
    per_write_leaves(g.sum_tree, g.min_tree, g.tree_cap, g.bidx, g.pri, g.B,
                     g.per_alpha, g.cnt);
    per_repair_paths(g.sum_tree, g.min_tree, g.tree_cap, g.B, 256,
                     [&](int i) { return g.tree_cap + g.bidx[i]; });
}

// CLIP (max_grad_norm > 0) adds, per net, the chunked sum of squares of the
// complete gradient slab and ONE more grid barrier between the dW phase and
// Adam; every one of the PNWG workgroups takes that barrier, under the
// template parameter alone (grid-uniform by construction, never data).
// k_step_persistent<false, false> is the kernel without any of it.
// QR (DIST_QUANTILE) swaps the three critic-family heads (critic,
// critic_target, the policy chain's critic) from softmax to identity and the
// projection/CE and policy-gradient rows for their quantile forms; phases,
// barriers and hand-offs are the same.  A template parameter like CLIP, so
// the categorical kernels carry no branch on it.
template <bool CLIP, bool QR>
__global__ void __launch_bounds__(256, 1)
k_step_persistent(StepArgs g, int nsteps) {
    constexpr int TW = (CLIP ? 1 : 0) + (QR ? 2 : 0);   // p_fwd / p_dw2 copy
    constexpr int HEAD = QR ? ACT_NONE : ACT_SOFTMAX;   // critic-family head
    __shared__ float lds[PLDS_FLOATS];
    unsigned long long tgt = g.gbar[160];   // cross-launch round base
    unsigned long long* ctr = g.gbar;
    int wg = blockIdx.x;
    // quad-barrier round base: my quad's arrival counter as of launch
    // entry (every member reads it before ANY member can arrive — the
    // first q_bar use sits behind several grid barriers)
    unsigned long long qrnd = ctr[192 + ((wg >> 2) << 4)];
    NetPtrs a = net_ptrs(g.p_actor, g.al);
    NetPtrs at = net_ptrs(g.p_actor_t, g.al);
    NetPtrs c = net_ptrs(g.p_critic, g.cl);
    NetPtrs ct = net_ptrs(g.p_critic_t, g.cl);
    const int O = g.O, A = g.A, H = g.H, K = g.K, B = g.B;

    // Schedule counters are read ONCE per launch and threaded through as
    // base+s (saves the per-step tick phase + its grid barrier, ~7 us);
    // wg 0 writes the advanced values back after the last step.
    const long long bt0 = g.cnt->beta_t;
    const long long ep0 = g.cnt->rng_epoch;
    const long long ta0 = g.cnt->adam_t_actor;
    const long long tc0 = g.cnt->adam_t_critic;
    // bs is double-buffered by step parity so the policy-block tail crew
    // can pre-sample the NEXT step's batch while this step's bs is still
    // read by the policy forward and the actor dW.  Parity derives from
    // the beta counter, so resume/relaunch stay deterministic.
    const int QW = ((B + 3) / 4) * 4;        // wgs used by the quad chains
    const bool otail = (QW + 32 <= PNWG) && (B <= 128);
    unsigned long long trnd = ctr[1280];
    const int pts = nsteps > 1 ? 1 : 0;      // the step PTIME stamps

    for (int s = 0; s < nsteps; ++s) {
        float* bs_cur = ((bt0 + s) & 1) ? g.bs_b : g.bs;
        float* bs_nxt = ((bt0 + s) & 1) ? g.bs : g.bs_b;
               PTIME(g, s, 0);
        // Steady-state (pipelined) step: at B <= 64 every step of a launch
        // but the first finds its batch sampled and its whole critic
        // forward (c_h1..c_h3, q) and ct_h1 already computed — the tail
        // crew did that under the previous step's policy block, after the
        // critic Adam made this step's critic weights final.  Such a step
        // skips PH0-PH4: the actor_t and actor forwards run inside the
        // quad phase below.  A launch's first step precomputed nothing
        // (parameter slabs and the replay may change between launches) and
        // takes PH0-PH4, as does every step at B > 64.
        const bool pipe = otail && s > 0;
        if (!pipe) {
            // PH0: PER sample + batch gather (only on a launch's first
            // step — at 64 < B <= 96 later steps were pre-sampled under
            // the previous actor-Adam)
            if (s == 0 || B > (PNWG - PNWG * 3 / 4) * 4) {
                p_sample(g, 0, ep0 + s, bt0 + s, bs_cur);
                p_bar(ctr, tgt);
            }
            PTIME(g, s, 1);
            // PH1: four independent L1s (16 wgs each)
            if (wg < PW4)
                p_fwd<TW>(lds, g.bs2, nullptr, at.w1, at.b1, g.at_h1, B, O, 0,
                      H, ACT_RELU, wg, PW4);
            else if (wg < 2 * PW4)
                p_fwd<TW>(lds, g.bs2, nullptr, ct.w1, ct.b1, g.ct_h1, B, O, 0,
                      H, ACT_RELU, wg - PW4, PW4);
            else if (wg < 3 * PW4)
                p_fwd<TW>(lds, bs_cur, nullptr, c.w1, c.b1, g.c_h1, B, O, 0, H,
                      ACT_RELU, wg - 2 * PW4, PW4);
            else
                p_fwd<TW>(lds, bs_cur, nullptr, a.w1, a.b1, g.pa_h1, B, O, 0, H,
                      ACT_RELU, wg - 3 * PW4, PW4);
            p_bar(ctr, tgt); PTIME(g, s, 2);
            // PH2: actor_t.L2 | critic.L2(cat h1, a) | actor.L2
            if (wg < PW3A)
                p_fwd<TW>(lds, g.at_h1, nullptr, at.w2, at.b2, g.at_h2, B, H, 0,
                      H, ACT_NONE, wg, PW3A);
            else if (wg < 2 * PW3A)
                p_fwd<TW>(lds, g.c_h1, g.ba, c.w2, c.b2, g.c_h2, B, H, A, H,
                      ACT_RELU, wg - PW3A, PW3A);
            else
                p_fwd<TW>(lds, g.pa_h1, nullptr, a.w2, a.b2, g.pa_h2, B, H, 0,
                      H, ACT_NONE, wg - 2 * PW3A, PW3B);
            p_bar(ctr, tgt); PTIME(g, s, 3);
            // PH3: L3s
            if (wg < PW3A)
                p_fwd<TW>(lds, g.at_h2, nullptr, at.w3, at.b3, g.at_h3, B, H, 0,
                      H, ACT_RELU, wg, PW3A);
            else if (wg < 2 * PW3A)
                p_fwd<TW>(lds, g.c_h2, nullptr, c.w3, c.b3, g.c_h3, B, H, 0, H,
                      ACT_RELU, wg - PW3A, PW3A);
            else
                p_fwd<TW>(lds, g.pa_h2, nullptr, a.w3, a.b3, g.pa_h3, B, H, 0,
                      H, ACT_RELU, wg - 2 * PW3A, PW3B);
            p_bar(ctr, tgt); PTIME(g, s, 4);
            // PH4: heads — actor_t tanh -> a2 | critic softmax -> q |
            //      actor tanh -> a_out
            if (wg < PW3A)
                p_fwd<TW>(lds, g.at_h3, nullptr, at.w4, at.b4, g.a2, B, H, 0, A,
                      ACT_TANH, wg, PW3A);
            else if (wg < 2 * PW3A)
                p_fwd<TW>(lds, g.c_h3, nullptr, c.w4, c.b4, g.q, B, H, 0, K,
                      HEAD, wg - PW3A, PW3A);
            else
                p_fwd<TW>(lds, g.pa_h3, nullptr, a.w4, a.b4, g.a_out, B, H, 0,
                      A, ACT_TANH, wg - 2 * PW3A, PW3B);
            // per-step loss accumulators zeroed here (grid barrier below
            // orders this before the quad-chained proj-CE / pgrad adds);
            // a pipelined step's were zeroed in the previous step's PH27
            if (wg == PNWG - 1 && threadIdx.x == 0) {
                g.cnt->loss_critic = 0.f;
                g.cnt->loss_actor = 0.f;
            }
            p_bar(ctr, tgt);
        } else {
            PTIME(g, s, 1); PTIME(g, s, 2); PTIME(g, s, 3); PTIME(g, s, 4);
        }
        PTIME(g, s, 5);
        // PH5-8 as ONE phase: the critic_target chain + projection + CE is
        // ROW-LOCAL (row b's p_t depends only on row b's ct_h1/a2), so each
        // quad of 4 wgs walks its 4-row group through ct.L2 -> ct.L3 ->
        // ct.L4 softmax -> C51 projection/CE with quad-local barriers; the
        // 16 quads never wait on each other (grid barriers cost ~3.3 us,
        // quad barriers well under 1 us, and straggler coupling is gone).
        // On a pipelined step the phase also carries what PH1-PH4 still
        // owe: actor_t's forward is row-local too, so each quad first
        // walks its rows through at.L1 -> at.L2 -> at.L3 -> at.L4 (tanh ->
        // a2), and beside the quads the 32 spare workgroups (the policy
        // block's tail crew) run the actor forward a.L1..L4 -> a_out over
        // the whole batch, crew barriers between the layers.  Both use the
        // weights the previous step's PH27 made final.
        {
            int q = wg >> 2, m = wg & 3;
            unsigned long long* qc = ctr + 192 + (q << 4);
            if (pipe && wg >= QW && wg < QW + 32) {
                p_fwd<TW>(lds, bs_cur, nullptr, a.w1, a.b1, g.pa_h1, B, O, 0, H,
                      ACT_RELU, wg - QW, 32);
                t_bar(ctr + 1280, trnd, 32);
                p_fwd<TW>(lds, g.pa_h1, nullptr, a.w2, a.b2, g.pa_h2, B, H, 0,
                      H, ACT_NONE, wg - QW, 32);
                t_bar(ctr + 1280, trnd, 32);
                p_fwd<TW>(lds, g.pa_h2, nullptr, a.w3, a.b3, g.pa_h3, B, H, 0,
                      H, ACT_RELU, wg - QW, 32);
                t_bar(ctr + 1280, trnd, 32);
                p_fwd<TW>(lds, g.pa_h3, nullptr, a.w4, a.b4, g.a_out, B, H, 0,
                      A, ACT_TANH, wg - QW, 32);
                PTIMEW(g, s, 53, QW);        // actor crew's end
            }
            for (int rg = q; rg < (B + 3) / 4; rg += PNWG / 4) {
                long r0 = (long)rg * 4;
                int nb = min(4, B - (int)r0);
                if (pipe) {
                    p_fwd<TW>(lds, g.bs2 + r0 * O, nullptr, at.w1, at.b1,
                          g.at_h1 + r0 * H, nb, O, 0, H, ACT_RELU, m, 4);
                    q_bar(qc, qrnd);
                    p_fwd<TW>(lds, g.at_h1 + r0 * H, nullptr, at.w2, at.b2,
                          g.at_h2 + r0 * H, nb, H, 0, H, ACT_NONE, m, 4);
                    q_bar(qc, qrnd);
                    p_fwd<TW>(lds, g.at_h2 + r0 * H, nullptr, at.w3, at.b3,
                          g.at_h3 + r0 * H, nb, H, 0, H, ACT_RELU, m, 4);
                    q_bar(qc, qrnd);
                    p_fwd<TW>(lds, g.at_h3 + r0 * H, nullptr, at.w4, at.b4,
                          g.a2 + r0 * A, nb, H, 0, A, ACT_TANH, m, 4);
                    q_bar(qc, qrnd); PTIME(g, s, 54);
                }
                p_fwd<TW>(lds, g.ct_h1 + r0 * H, g.a2 + r0 * A, ct.w2, ct.b2,
                      g.ct_h2 + r0 * H, nb, H, A, H, ACT_RELU, m, 4);
                q_bar(qc, qrnd);
                p_fwd<TW>(lds, g.ct_h2 + r0 * H, nullptr, ct.w3, ct.b3,
                      g.ct_h3 + r0 * H, nb, H, 0, H, ACT_RELU, m, 4);
                q_bar(qc, qrnd);
                p_fwd<TW>(lds, g.ct_h3 + r0 * H, nullptr, ct.w4, ct.b4,
                      g.p_t + r0 * K, nb, H, 0, K, HEAD, m, 4);
                if (m == 0)
                    p_project_ce<QR>(g, lds, (int)r0);
                PTIME(g, s, 55);
                // no trailing q_bar: row groups are independent and the
                // closing grid barrier publishes everything
            }
        }
        p_bar(ctr, tgt);
        PTIME(g, s, 6); PTIME(g, s, 7); PTIME(g, s, 8); PTIME(g, s, 9);
        // PH10-12 as ONE phase: critic dX chain (pre-update weights),
        // row-local — quad-chained like the target block above
        {
            int q = wg >> 2, m = wg & 3;
            unsigned long long* qc = ctr + 192 + (q << 4);
            // this step's PER write-back rides on the first spare
            // workgroup (B <= 64): the priorities have been final since
            // the CE row, nothing reads the trees before the tail crew's
            // sample two grid barriers on, and the ~20 us single-workgroup
            // job no longer heads the tail crew's serial chain
            if (otail) p_per_update(g, QW);
            for (int rg = q; rg < (B + 3) / 4; rg += PNWG / 4) {
                long r0 = (long)rg * 4;
                int nb = min(4, B - (int)r0);
                p_bwd_dx(lds, g.dlog + r0 * K, c.w4, 0, H, K, nb,
                         g.c_h3 + r0 * H, ACT_RELU, g.d3 + r0 * H, m, 4);
                q_bar(qc, qrnd);
                p_bwd_dx(lds, g.d3 + r0 * H, c.w3, 0, H, H, nb,
                         g.c_h2 + r0 * H, ACT_RELU, g.d2 + r0 * H, m, 4);
                q_bar(qc, qrnd);
                p_bwd_dx(lds, g.d2 + r0 * H, c.w2, 0, H, H, nb,
                         g.c_h1 + r0 * H, ACT_RELU, g.d1 + r0 * H, m, 4);
            }
        }
        p_bar(ctr, tgt);
        PTIME(g, s, 10); PTIME(g, s, 11); PTIME(g, s, 12);
        // PH13: critic dW, 4 jobs split by tile count (l1 is the biggest)
        if (wg < PNWG / 16)
            p_dw2<TW>(lds, g.d1, bs_cur, nullptr, g.g_critic + g.cl[0].w_off,
                 g.g_critic + g.cl[0].b_off, B, O, 0, H, wg, PNWG / 16);
        else if (wg < PNWG / 2)
            p_dw2<TW>(lds, g.d2, g.c_h1, g.ba, g.g_critic + g.cl[1].w_off,
                 g.g_critic + g.cl[1].b_off, B, H, A, H, wg - PNWG / 16,
                 PNWG / 2 - PNWG / 16);
        else if (wg < PNWG * 7 / 8)
            p_dw2<TW>(lds, g.d3, g.c_h2, nullptr, g.g_critic + g.cl[2].w_off,
                 g.g_critic + g.cl[2].b_off, B, H, 0, H, wg - PNWG / 2,
                 PNWG * 7 / 8 - PNWG / 2);
        else
            p_dw2<TW>(lds, g.dlog, g.c_h3, nullptr, g.g_critic + g.cl[3].w_off,
                 g.g_critic + g.cl[3].b_off, B, H, 0, K, wg - PNWG * 7 / 8,
                 PNWG - PNWG * 7 / 8);
        p_bar(ctr, tgt); PTIME(g, s, 13);
        // PH13b (clip-on only): |g_critic|^2 by chunks, all workgroups
        float csc = 1.f;
        if (CLIP) {
            p_grad_sumsq(g.g_critic, g.n_critic, g.gn_part_c, lds);
            p_bar(ctr, tgt); PTIME(g, s, 56);
            csc = p_grad_scale(g, 0);
        }
        // PH14: Adam + target soft-update, critic
        p_adam_lerp<CLIP>(g.p_critic, g.g_critic, g.m_critic, g.v_critic,
                          g.p_critic_t, g.n_critic, g.lr_critic, g.tau,
                          tc0 + s, csc);
        p_bar(ctr, tgt); PTIME(g, s, 14);
        // PH15-25 as ONE phase: the whole policy megachain — critic(s,
        // a_out) forward with UPDATED critic params, policy head gradient,
        // dX back through the critic to the action slice, then dX through
        // the actor — is row-local end-to-end, so each quad chains its
        // 4-row group through all 10 layers with quad-local barriers
        // (replaces 11 grid barriers; VERDICT r1 #7 / NOTES.md roadmap —
        // this is the pair-barrier idea at quad granularity, which keeps
        // the weight re-streaming of the tiled form: one full W read per
        // row-group, L2-resident)
        {
            int q = wg >> 2, m = wg & 3;
            unsigned long long* qc = ctr + 192 + (q << 4);
            if (otail && wg >= QW && wg < QW + 32) {
                // tail crew (32 spare wgs): the NEXT step's sample (the
                // trees were repaired in the critic dX phase), its ct L1
                // and its whole critic forward — hidden under the policy
                // megachain.  It precomputes nothing on a launch's last
                // step, so nothing precomputed crosses a launch boundary.
                // Safe: bs2/ba/br/bd/bw/bidx of step s were fully consumed
                // before this block; bs_nxt is the other bs buffer.
                if (s + 1 < nsteps) {
                    p_sample(g, QW, ep0 + s + 1, bt0 + s + 1, bs_nxt);
                    t_bar(ctr + 1280, trnd, 32);
                    p_fwd<TW>(lds, g.bs2, nullptr, ct.w1, ct.b1, g.ct_h1, B,
                          O, 0, H, ACT_RELU, wg - QW, 32);
                    p_fwd<TW>(lds, bs_nxt, nullptr, c.w1, c.b1, g.c_h1, B, O,
                          0, H, ACT_RELU, wg - QW, 32);
                    // ... and the rest of the NEXT step's critic forward:
                    // the critic's weights have been final since PH14,
                    // ba is the next step's since the sample above, and
                    // this step's last readers of c_h* and q (PH13, the
                    // CE row) are long past
                    t_bar(ctr + 1280, trnd, 32);
                    p_fwd<TW>(lds, g.c_h1, g.ba, c.w2, c.b2, g.c_h2, B, H, A,
                          H, ACT_RELU, wg - QW, 32);
                    t_bar(ctr + 1280, trnd, 32);
                    p_fwd<TW>(lds, g.c_h2, nullptr, c.w3, c.b3, g.c_h3, B, H,
                          0, H, ACT_RELU, wg - QW, 32);
                    t_bar(ctr + 1280, trnd, 32);
                    p_fwd<TW>(lds, g.c_h3, nullptr, c.w4, c.b4, g.q, B, H, 0,
                          K, HEAD, wg - QW, 32);
                }
                PTIMEW(g, s, 52, QW);        // tail crew's end
            }
            for (int rg = q; rg < (B + 3) / 4; rg += PNWG / 4) {
                long r0 = (long)rg * 4;
                int nb = min(4, B - (int)r0);
                PTIME(g, s, 40);
                p_fwd<TW>(lds, bs_cur + r0 * O, nullptr, c.w1, c.b1,
                      g.pc_h1 + r0 * H, nb, O, 0, H, ACT_RELU, m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 41);
                p_fwd<TW>(lds, g.pc_h1 + r0 * H, g.a_out + r0 * A, c.w2, c.b2,
                      g.pc_h2 + r0 * H, nb, H, A, H, ACT_RELU, m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 42);
                p_fwd<TW>(lds, g.pc_h2 + r0 * H, nullptr, c.w3, c.b3,
                      g.pc_h3 + r0 * H, nb, H, 0, H, ACT_RELU, m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 43);
                p_fwd<TW>(lds, g.pc_h3 + r0 * H, nullptr, c.w4, c.b4,
                      g.pq + r0 * K, nb, H, 0, K, HEAD, m, 4);
                if (m == 0)
                    p_policy_grad<QR>(g, (int)r0);
                q_bar(qc, qrnd); PTIME(g, s, 44);
                p_bwd_dx(lds, g.pd3 + r0 * K, c.w4, 0, H, K, nb,
                         g.pc_h3 + r0 * H, ACT_RELU, g.pd2 + r0 * H, m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 45);
                p_bwd_dx(lds, g.pd2 + r0 * H, c.w3, 0, H, H, nb,
                         g.pc_h2 + r0 * H, ACT_RELU, g.pdh1 + r0 * H,
                         m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 46);
                if (m == 0)
                    p_bwd_dx_narrow(g, g.pdh1, c.w2, H, H + A, H,
                                    g.a_out, g.adz, (int)r0);
                q_bar(qc, qrnd); PTIME(g, s, 47);
                p_bwd_dx(lds, g.adz + r0 * A, a.w4, 0, H, A, nb,
                         g.pa_h3 + r0 * H, ACT_RELU, g.az3 + r0 * H, m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 48);
                p_bwd_dx(lds, g.az3 + r0 * H, a.w3, 0, H, H, nb,
                         nullptr, ACT_NONE, g.az2 + r0 * H, m, 4);
                q_bar(qc, qrnd); PTIME(g, s, 49);
                p_bwd_dx(lds, g.az2 + r0 * H, a.w2, 0, H, H, nb,
                         g.pa_h1 + r0 * H, ACT_RELU, g.az1 + r0 * H, m, 4);
                PTIME(g, s, 51);
            }
        }
        p_bar(ctr, tgt);
        PTIME(g, s, 15); PTIME(g, s, 16); PTIME(g, s, 17);
        PTIME(g, s, 18); PTIME(g, s, 19); PTIME(g, s, 20);
        PTIME(g, s, 21); PTIME(g, s, 22); PTIME(g, s, 23);
        PTIME(g, s, 24); PTIME(g, s, 25);
        // PH26: actor dW, with the PER tree write-back overlapped on the
        // last workgroup (priorities have been final since the proj+CE
        // phase; the counter tick moves to the final phase so both Adams
        // still read this step's t)
        if (wg < PNWG / 16)
            p_dw2<TW>(lds, g.az1, bs_cur, nullptr, g.g_actor + g.al[0].w_off,
                 g.g_actor + g.al[0].b_off, B, O, 0, H, wg, PNWG / 16);
        else if (wg < PNWG * 15 / 32)
            p_dw2<TW>(lds, g.az2, g.pa_h1, nullptr, g.g_actor + g.al[1].w_off,
                 g.g_actor + g.al[1].b_off, B, H, 0, H, wg - PNWG / 16,
                 PNWG * 15 / 32 - PNWG / 16);
        else if (wg < PNWG * 7 / 8)
            p_dw2<TW>(lds, g.az3, g.pa_h2, nullptr, g.g_actor + g.al[2].w_off,
                 g.g_actor + g.al[2].b_off, B, H, 0, H, wg - PNWG * 15 / 32,
                 PNWG * 7 / 8 - PNWG * 15 / 32);
        else if (wg < PNWG - 2)
            p_dw2<TW>(lds, g.adz, g.pa_h3, nullptr, g.g_actor + g.al[3].w_off,
                 g.g_actor + g.al[3].b_off, B, H, 0, A, wg - PNWG * 7 / 8,
                 PNWG - 2 - PNWG * 7 / 8);
        else if (!otail && wg == PNWG - 1)
            p_per_update(g, PNWG - 1);   // PH10-12 did it when otail
        p_bar(ctr, tgt); PTIME(g, s, 26);
        // PH26b (clip-on only): |g_actor|^2 by chunks.  ALL workgroups take
        // the phase and its barrier, the ones that sample in PH27 included
        if (CLIP) {
            p_grad_sumsq(g.g_actor, g.n_actor, g.gn_part_a, lds);
            p_bar(ctr, tgt); PTIME(g, s, 57);
        }
        // PH27: Adam + soft-update, actor (wgs 0-47) overlapped with the
        // NEXT step's PER sample + gather (wgs 48-63; tree was repaired in
        // PH26, schedule counters offset by the pending tick)
        {
            int anw = otail ? PNWG : PNWG * 3 / 4;
            if (wg < anw)
                p_adam_lerp<CLIP>(g.p_actor, g.g_actor, g.m_actor,
                                  g.v_actor, g.p_actor_t, g.n_actor,
                                  g.lr_actor, g.tau, ta0 + s,
                                  CLIP ? p_grad_scale(g, 1) : 1.f, anw);
            else if (s + 1 < nsteps && B <= (PNWG - PNWG * 3 / 4) * 4)
                p_sample(g, PNWG * 3 / 4, ep0 + s + 1, bt0 + s + 1, bs_nxt);
            // the next step is pipelined and has no PH4: zero its loss
            // accumulators here (this step's are complete; the barrier
            // below orders the zeroes before the next proj-CE adds)
            if (otail && s + 1 < nsteps && wg == PNWG - 1
                && threadIdx.x == 0) {
                g.cnt->loss_critic = 0.f;
                g.cnt->loss_actor = 0.f;
            }
        }
        p_bar(ctr, tgt); PTIME(g, s, 27); PTIME(g, s, 28);
        // (the per-step schedule-counter tick phase is gone: counters were
        // hoisted to base+s registers; final values land below)
    }
    if (wg == 0 && threadIdx.x == 0) {
        g.cnt->beta_t = bt0 + nsteps;
        g.cnt->rng_epoch = ep0 + nsteps;
        g.cnt->adam_t_actor = ta0 + nsteps;
        g.cnt->adam_t_critic = tc0 + nsteps;
        g.gbar[160] = tgt;
    }
}

}  // namespace d4pg
