// Device-side primitives shared by the gfx950 kernels of libgpe_hip.so (not part of the C ABI): vector typedefs, the split of an
// fp32 pair into 16-bit terms, the samplers' counter-based random numbers, the inter-workgroup hand-off, the recurrent state scale
// and the LSTM cell.  A new persistent kernel starts from these instead of growing its own copies.
#pragma once
#include "gpe_common.h"
#include <math.h>

typedef _Float16 gpe_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 gpe_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gpe_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 gpe_bf16x8 __attribute__((ext_vector_type(8)));
typedef float gpe_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned gpe_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned gpe_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gpe_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- split of an fp32 pair into 16-bit terms ------------------------------------------------------------------------------
// f16x3 mode: (a, b) = h + l in two fp16 terms each (11 + 11 bits + the sign of l = 23), packed as {a | b << 16}.  The caller
// has brought the operand into fp16's range by a power of two (gpe_h3_scale_of, GPE_STATE_SA); the residual is exact in fp32.
__device__ __forceinline__ void gpe_split2_f16(float a, float b, unsigned& h, unsigned& l)
{
    const gpe_f32x2 v = {a, b};
    const gpe_f16x2 hh = __builtin_convertvector(v, gpe_f16x2);                    // v_cvt_pk_f16_f32, RNE
    const gpe_f32x2 r = v - __builtin_convertvector(hh, gpe_f32x2);
    h = __builtin_bit_cast(unsigned, hh);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(r, gpe_f16x2));
}
// ... of (a s, b s), s the operand's power of two
__device__ __forceinline__ void gpe_split2_f16(float a, float b, float s, unsigned& h, unsigned& l) { gpe_split2_f16(a * s, b * s, h, l); }

// bf16 modes: {bf16(a) | bf16(b) << 16}, RNE (v_cvt_pk_bf16_f32), and the two-term split built on it (fp32's exponent range:
// no scale)
__device__ __forceinline__ unsigned gpe_cvt2_bf16(float a, float b)
{
    const gpe_f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, gpe_bf16x2));
}
__device__ __forceinline__ void gpe_split2_bf16(float a, float b, unsigned& h, unsigned& l)
{
    h = gpe_cvt2_bf16(a, b);
    l = gpe_cvt2_bf16(a - __uint_as_float(h << 16), b - __uint_as_float(h & 0xffff0000u));
}

// ---- recurrent state scale ------------------------------------------------------------------------------------------------
// The recurrent state enters the fp16 pipe scaled by 2^12: |h| < 1 for every state an LSTM / GRU cell produces (o * tanh(c);
// a convex combination of tanh values), start states up to |h0| < 16 stay finite, and a state down to 3e-5 keeps both terms
// normal (smaller ones keep an absolute error < 1.5e-8).  Callers of the f16x3 recurrences guarantee |h0| < 16.
#define GPE_STATE_SA 4096.f
#define GPE_STATE_INV_SA (1.f / 4096.f)

// ---- counter-based random numbers --------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ gpe_u32x4 gpe_philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return gpe_u32x4{c0, c1, c2, c3};
}
// the samplers' block of one decision: key = the seed, counter = (item | kind << 28, attempt | b << 8, draw lo, draw hi), b the batch
// slot (b8 = b << 8).  The kinds in use: 0 .. 4 gpe_stitch_sample.hip, 8 and 9 gpe_mesh_sample.hip, 10 .. 12 gpe_epoch_feed.hip
// (there the state's second word is the epoch, and b is a slot of a batch: include/gpe_hip_feed.h), 13 gpe_scan_sample.hip
struct gpe_rng {
    unsigned k0, k1, d0, d1, b8;
    __device__ __forceinline__ gpe_u32x4 operator()(int kind, unsigned item, unsigned attempt = 0) const
    {
        return gpe_philox4x32(item | ((unsigned)kind << 28), attempt | b8, d0, d1, k0, k1);
    }
};

// ---- inter-workgroup hand-off inside one launch ---------------------------------------------------------------------------
// Recipe R1 (MI355X_MICROARCH.md "Workgroup dispatch, XCD placement & inter-workgroup visibility"; cdna_hip_programming.md
// Guideline 16):
//   producer: the payload leaves in sc1 (write-through) stores; EVERY storing wave drains vmcnt; then ONE lane makes ONE relaxed
//             agent-scope increment of the arrival counter;
//   consumer: polls the counter with relaxed agent-scope loads (sc1: served by L2 / the fabric, never by the CU's L1) and reads
//             the payload with sc1 loads below the poll — the producer stored sc1, so no acquire fence.
// Nothing depends on workgroup -> XCD placement or dispatch order.  Residency: a wait only ends if its producer runs, so ALL
// workgroups of the launch must be co-resident (the host sizes the grid to what the chip holds at once) — unless, as with the
// last-arriver ticket, nobody waits.  Every wait is bounded and traps: a stuck workgroup must not hang the queue.  Counters are
// zeroed on the stream in front of every launch.
#define GPE_SPIN_LIMIT (1u << 23)  // polls (>= 0.1 us each) before a stuck wave traps

// one look at a counter: the load alone (per lane; a caller that looks at the value later keeps the latency off its path) ...
__device__ __forceinline__ unsigned gpe_flag_load(const unsigned* flag)
{
    return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... and its wave-uniform value
__device__ __forceinline__ unsigned gpe_flag_poll(const unsigned* flag) { return __builtin_amdgcn_readfirstlane(gpe_flag_load(flag)); }
// every wave waits for itself
__device__ __forceinline__ void gpe_flag_wait(const unsigned* flag, unsigned need)
{
    unsigned spins = 0;
    while (gpe_flag_poll(flag) < need) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > GPE_SPIN_LIMIT) __builtin_trap();
    }
    asm volatile("" ::: "memory");           // payload loads stay below the poll
}
// this wave's stores have left
__device__ __forceinline__ void gpe_drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// THE increment (one lane calls it, after the drains); its return value is the caller's ticket: how many arrived before it
__device__ __forceinline__ unsigned gpe_flag_ticket(unsigned* flag)
{
    return __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// arrive, wave form: the calling wave stored the whole payload
__device__ __forceinline__ void gpe_flag_arrive_wave(unsigned* flag)
{
    gpe_drain_stores();
    if ((threadIdx.x & 63) == 0) gpe_flag_ticket(flag);
}
// arrive, workgroup form: every wave may have stored; a barrier between the drains and the increment (called by all threads).
// stamp: optional wall-clock word written when thread 0 has drained (measurement aid)
__device__ __forceinline__ void gpe_flag_arrive_wg(unsigned* flag, unsigned long long* stamp = nullptr)
{
    gpe_drain_stores();
    if (stamp && threadIdx.x == 0) *stamp = wall_clock64();
    __syncthreads();
    if (threadIdx.x == 0) gpe_flag_ticket(flag);
}
// (A last-arriver protocol — gpe_rnn_wave_splitk_kernel — is the workgroup form with the ticket handed round through LDS: nobody
// waits, the workgroup that draws the last ticket reads the others' payload itself, with sc1 loads.)

// ---- LSTM cell (gate order i, f, g, o as in torch.nn.LSTM) -----------------------------------------------------------------
// forward: the four pre-activations and c_{t-1} -> activated gates and c_t, then h_t from them (gpe_lstm_cell_h).  Two calls, so that
// a caller can put its gate and c stores in front of tanh(c_t), whose branches end the basic block (all but gpe_rnn_persist_mt do).
// The pre-activations come finished, or as (z, addend) pairs that are added here, each right in front of its activation: what a
// kernel wrote before the cell was shared, and the order decides its schedule and which product of c_t the compiler fuses
template <bool ADD>
__device__ __forceinline__ void gpe_lstm_cell_fwd_(float zi, float zf, float zg, float zo, float ei, float ef, float eg, float eo,
                                                   float c_prev, float& ig, float& fg, float& gg, float& og, float& c)
{
    ig = gpe_sigmoid(ADD ? zi + ei : zi);
    fg = gpe_sigmoid(ADD ? zf + ef : zf);
    gg = tanhf(ADD ? zg + eg : zg);
    og = gpe_sigmoid(ADD ? zo + eo : zo);
    c = fg * c_prev + ig * gg;
}
__device__ __forceinline__ void gpe_lstm_cell_fwd(float zi, float zf, float zg, float zo, float c_prev, float& ig, float& fg,
                                                  float& gg, float& og, float& c)
{
    gpe_lstm_cell_fwd_<false>(zi, zf, zg, zo, 0.f, 0.f, 0.f, 0.f, c_prev, ig, fg, gg, og, c);
}
__device__ __forceinline__ void gpe_lstm_cell_fwd(float zi, float ei, float zf, float ef, float zg, float eg, float zo, float eo,
                                                  float c_prev, float& ig, float& fg, float& gg, float& og, float& c)
{
    gpe_lstm_cell_fwd_<true>(zi, zf, zg, zo, ei, ef, eg, eo, c_prev, ig, fg, gg, og, c);
}
__device__ __forceinline__ float gpe_lstm_cell_h(float og, float c) { return og * tanhf(c); }
// backward: saved gates, c_t, c_{t-1}, dh_t and the carry dc_{t+1} f_{t+1} (carry_in, NULL = none) -> the four pre-activation
// gradients and the carry dc_t f_t
__device__ __forceinline__ void gpe_lstm_cell_bwd(float ig, float fg, float gg, float og, float c, float c_prev, float dh,
                                                  const float* carry_in, float& di, float& df, float& dg, float& dgo,
                                                  float& carry_out)
{
    const float tc = tanhf(c);
    float dc = dh * og * (1.f - tc * tc);
    if (carry_in) dc += *carry_in;
    di = dc * gg * ig * (1.f - ig);
    df = dc * c_prev * fg * (1.f - fg);
    dg = dc * ig * (1.f - gg * gg);
    dgo = dh * tc * og * (1.f - og);
    carry_out = dc * fg;
}

// ---- sparsemax row width ------------------------------------------------------------------------------------------------------
// sparsemax over rows of width W <= 32: one row per lane, the row sorted in registers by a fully unrolled odd-even transposition
// network of this many entries (gpe_pool.hip: forward; gpe_loss.hip: the sparsemax loss runs the same sort)
#define SPX_W 32

// ---- weight slice -> LDS ----------------------------------------------------------------------------------------------------
// copy columns [c0, c0 + CW) of every 16-byte-piece group of a packed weight into LDS with NTHR threads: piece (group, c) of the
// pack sits at (group * Npad + c0 + c) * 16 bytes
template <int CW, int NTHR>
__device__ __forceinline__ void gpe_fill(char* dst, const void* src, int ngroups, int Npad, int c0)
{
    const gpe_u32x4* s = reinterpret_cast<const gpe_u32x4*>(src);
    gpe_u32x4* d = reinterpret_cast<gpe_u32x4*>(dst);
    const int total = ngroups * CW;
    for (int e = threadIdx.x; e < total; e += NTHR) {
        const int grp = e / CW, c = e - grp * CW;
        d[e] = s[(long)grp * Npad + c0 + c];
    }
}
