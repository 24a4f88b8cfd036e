// pt_hip_queue.h -- the segmented queues' device primitives: workgroup shape, wave-uniform slot counters, the ticket counters that
// hand queue segments to persistent waves, the per-round flags.  (pt_hip_*.h: read by hipcc only, as parts of ptrs_hip.hip's one
// translation unit, in its order; the CPU twins never include them.)
#pragma once

constexpr int BLOCK = 256, WAVES = BLOCK / 64;

// Segmented queues, one WAVE per segment.  Every queue of a pass is split into G segments; the wave that consumes segment s of
// one stage appends only to segment s of the next, so a segment has one writer at a time and its slots come from a counter the
// wave keeps in a scalar register (one s_bcnt1 per push): no atomics on the data path at all, neither global (the first version:
// ~16 M returning atomics per frame on one address) nor LDS (round 2: one ds_add per wave and push, plus a workgroup barrier
// per segment).  The queue kernels are PERSISTENT: a launch holds only as many workgroups as fit the machine at once
// (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs), and each of their waves takes segment numbers from a per-launch ticket
// counter until the G segments are gone (one returning global atomic per wave and segment, asked for one segment ahead).  With a
// workgroup per segment and G = 2048 workgroups on 5-7 resident per CU, the second scheduling round of every launch ran a third
// full (time-average occupancy 8 / ceil(8 / c) waves per SIMD); now every wave slot works until the tickets run out, and the
// tail is one wave-segment (G / resident waves is 1.3-2.7 at the default grid_mult).
__device__ inline uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ inline uint32_t lanes_below(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); } // set bits of m below this lane
__device__ inline uint32_t wave_push(uint32_t &count, bool pred) { // slot for every lane with pred; count is wave-uniform
    const unsigned long long m = __ballot(pred);
    const uint32_t slot = count + lanes_below(m);
    count += (uint32_t)__popcll(m);
    return slot;
}
__device__ inline uint32_t wave_of_launch() { return blockIdx.x * WAVES + (threadIdx.x >> 6); } // the wave's number in its launch: its segment where waves are mapped without tickets, its home counter (mod TK_SUB) with them
// The segment a wave works on next, or a number >= G when the launch has none left.  One counter for the whole launch would take one
// returning atomic per segment on ONE address, ~18 ns apiece on MI355X: 0.3 ms for G = 16384, which is what a kernel of the thin late
// rounds of a pass then costs however little it has to do (measured: 11 of Cornell's 16 rounds, 30 ms of a 200 ms frame).  So the
// launch has TK_SUB counters 128 bytes apart, each handing out a contiguous range of ceil(G / TK_SUB) segments; a wave reads all of
// them with one load (lane k reads counter k), takes a ticket from the first open one at or after its home counter, and moves on as
// ranges run out.  The atomics of a launch spread over TK_SUB addresses, and a wave sees the launch exhausted with a single load.
enum : uint32_t { TK_SUB = 64, TK_SUB_STRIDE = 32, TK_LAUNCH_WORDS = TK_SUB * TK_SUB_STRIDE };
__device__ inline uint32_t seg_next(uint32_t *ticket, uint32_t G) {
    const uint32_t per = (G + TK_SUB - 1u) / TK_SUB; // every counter hands out `per` numbers; those at or beyond G (the last counters' surplus) are skipped
    const uint32_t home = wave_of_launch() & (TK_SUB - 1u);
    for (;;) {
        // lane k reads counter k (a device-coherent load: the counters only grow, a stale value costs one atomic that comes back empty); which
        // counters are still open is a lane mask.  In one asm statement with one temporary: written in C++ the scan's per-lane values are
        // hoisted out of the callers' segment loops and cost every kernel ~10 vector registers.
        uint32_t tmp; unsigned long long open;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshlrev_b32 %0, 7, %0\n\tglobal_load_dword %0, %0, %2 sc1\n\ts_waitcnt vmcnt(0)\n\tv_cmp_gt_u32 %1, %3, %0"
                     : "=&v"(tmp), "=s"(open) : "s"(ticket), "s"(per) : "memory");
        static_assert(TK_SUB_STRIDE * 4u == 128u, "the asm above shifts the lane id by 7");
        if (open == 0ull) return 0xffffffffu;
        const unsigned long long rot = home ? ((open >> home) | (open << (64u - home))) : open; // the home counter first
        const uint32_t c = (home + (uint32_t)__ffsll((long long)rot) - 1u) & (TK_SUB - 1u);
        uint32_t t = 0;
        if (__lane_id() == 0) t = atomicAdd(ticket + c * TK_SUB_STRIDE, 1u);
        t = rfl(t);
        const uint32_t s = c * per + t;
        if (t < per && s < G) return s;
        // the counter ran out between the load and the atomic, or the number is one of its surplus: look again
    }
}
// counts[(row * Q_STRIDE + q) * G + s]
__device__ inline uint32_t *seg_count(const DQueues &Q, uint32_t row, int q, uint32_t G, uint32_t s) { return Q.counts + ((size_t)row * Q_STRIDE + (size_t)q) * G + s; }
enum { TK_EXTEND = 0, TK_CONNECT = 1, TK_SHADE0 = 2, TK_EPILOGUE = 9, TK_RESOLVE = 10, TK_PRESAMPLE = 11, TK_TAIL = 12 }; // tickets[(row * Q_STRIDE + TK_*) * TK_LAUNCH_WORDS]: the counters of one launch of a pass
// A round nobody reaches (every path has ended: rounds are enqueued without asking, and for scenes with null-BSDF skips a few more
// than max_depth + 1) costs its launches only: each kernel looks at the flag and leaves.
// (Q.alive[row]: the round's "some path is still alive" flag, set by the shade kernels of the round before)
__device__ inline bool round_is_dead(const DQueues &Q, uint32_t it) { return it > 0u && rfl(Q.alive[it]) == 0u; }
