// k_xspec for 2048-bin rows whose template keeps fewer than 512 harmonics (MODE 2,
// noise given or measured): the benchmark shape, built on the one-exchange FFT of pp_fftq.h.
//
// Same contract as k_xspec<1024, Tin, TAIL, 2> (pp_kernels.h).  What differs is the
// path of the row through the LDS, which is the unit this kernel saturates (one LDS
// per CU, eight resident rows; see pp_fftq.h):
//
//   k_xspec          stage-1 store, stage-2 load + store, stage-3 load + store,
//                    split loads (k and M - k)                    110 ds_*_b128 per row
//   this kernel      one 16 x 16 transpose (16 + 16), then the split reads only the
//                    PARTNERS: lane t ends with Z[lam + 64 kd] in register kd and works
//                    on harmonics k = lam + 64 j (j = 0..6) -- Z_k is already in its
//                    registers; Z_{M-k} = Z[(64 - lam) + 64 (15 - j)] sits in register
//                    15 - j of the lane that owns 64 - lam, so every lane publishes its
//                    registers 9..15 and reads seven values back     46 per row
//
// The lane that owns lam = 0 has no harmonic 0 to work on (F0_fact = 0): it takes
// k = 64 (j + 1) instead, from its registers 1..7, and is its own partner.  Both
// exchanges are free of bank conflicts: the transpose writes with a pitch of 17
// elements and reads contiguously; the partner map sends every aligned group of eight
// lanes to eight lanes with distinct low three bits.
#pragma once
#include "pp_fftq.h"

// The harmonics a lane works on come in slots of 64 (k = kb + 64 j) and a channel's template keeps a PREFIX of them
// (kt_n is a multiple of 64, wave-uniform).  The slot loop ends with the last kept slot instead of walking the dropped
// ones for their two recurrences (split twiddle W^k and phasor e^{i kappa phi}: 8 f64 instructions a slot) and their
// partner read from LDS: the example template keeps 4.5 of 7 (of 8 at 1024 bins) slots on average.  Same sums, same
// bits (profiles/r05_slot_exit_ab.txt).  Every slot's partner register is published, kept or not: publishing only the
// kept ones costs a scalar jump that eats what the stores save (profiles/r05_publish_kept_ab.txt).

namespace pp {

// a wave asks for its ticket after a wave-specific number of rows, uniform over this fraction of its share of the launch
// (every wave asks, the first `tickets` to ask get one: with 3/4 and four waves per ticket they are gone after the first fifth)
constexpr unsigned PP_TICKET_WINDOW_NUM = 3u, PP_TICKET_WINDOW_DEN = 4u;
// (CU: the wave is one of a workgroup's eight and counts as a one-wave workgroup, see RowWalk)
template <bool CU = false>
__device__ __forceinline__ int ticket_moment(const long long nrows) {
    const unsigned share = (unsigned)(nrows / (long long)RowWalk<true, CU>::walkers()) + 1u;
    return 1 + (int)(((RowWalk<true, CU>::me() * 2654435761u) >> 8) % (share * PP_TICKET_WINDOW_NUM / PP_TICKET_WINDOW_DEN + 1u));
}

// where the row after this one starts: (subint i_nx of the list, channel n_nx of the subset), or this row again (rc)
// when the walk has run out -- the prefetch is unconditional
template <int M, typename Tin>
__device__ __forceinline__ const Tin* next_row_of(const XspecArgs& a, const unsigned more_nx, const int i_nx, const int n_nx,
                                                  const size_t rc) {
    const size_t rn = more_nx ? (size_t)sub_of(a.act, i_nx) * a.nchan_full + (a.coff + n_nx * a.cstep) : rc;
    return reinterpret_cast<const Tin*>(a.data) + rn * (2 * M);
}

// the free element of the transpose image (pitch 17: element 16 of every lane's run is never written or read) of lane
// l of the LAST row of 16 lanes -- beyond what the partner exchange (elements 0..447, 0..767 when the noise is measured)
// and the reduction publish
constexpr int FFTQ_FREE_ELEM0 = 3 * 272 + 16, FFTQ_FREE_PITCH = 17;

// The results of a row -- the 12 Taylor sums, S_d and (TAIL) the measured noise, wave totals as wave_reduce_lds leaves
// them -- to memory.  All four lanes of quad q hold total q and the quads past the last total hold the last one, so EVERY
// lane has a value and a place for it: the results leave in ONE store that no branch skips, and the compiler can count
// it.  (Stores that only some lanes issue are branched around when none does; behind them the number of accesses in
// flight is unknown, and the next row's wait for its data has to be one for the store's acknowledgement as well.)
// ONE = false (the kernels that also measure the noise): the two or three one-lane stores.
// LEAN (ONE, noise given): the sign of total q <= 10 is bit 1 of q + 1 (+ - - + + - - + + - -, and + for the remainder
// coefficient), added to the high dword as (x << 31) instead of a negated copy chosen by two compares; the Taylor
// sums' address is formed for every q and replaced as a whole for S_d.  The same values to the same places.
template <int M, bool TAIL, bool ONE = true, bool LEAN = false>
__device__ __forceinline__ void store_row_results(const XspecArgs& a, const size_t rc, const int tid, double tv) {
    constexpr int H = M + 1, kc = (int)(0.75 * H);   // get_noise_PS: int((1 - 1/4) * len(pows))
  if constexpr (ONE && LEAN) {
    static_assert(!TAIL && PP_TJ == 10 && PP_TSTRIDE == 12, "sign pattern of totals 0..11; S_d in the quads behind them");
    const unsigned q = (unsigned)wave_reduce16_index(tid);
    const double th = 0.5 * tv;
    double val = __hiloint2double((int)((unsigned)__double2hiint(th) + (((q + 1u) >> 1) << 31)), __double2loint(th));
    double* dst = a.tay + tay_idx(rc, 0) + q;
    if (q >= (unsigned)PP_TSTRIDE) { val = tv; dst = a.sdraw + rc; }
    typedef double __attribute__((address_space(1)))* gdp_t;
    *(gdp_t)(uintptr_t)dst = val;
  } else if constexpr (ONE) {
    const int q = wave_reduce16_index(tid);
    const double th = 0.5 * tv;
    // Re(i^q z): +Re, -Im, -Re, +Im, ...   (x 1/2: unhalved template against 2 d_k)
    double val = (q <= PP_TJ && ((q & 3) == 1 || (q & 3) == 2)) ? -th : th;
    double* dst = a.tay + tay_idx(rc, q < PP_TSTRIDE ? q : 0);
    if (q >= PP_TSTRIDE) { val = tv; dst = a.sdraw + rc; }
    if (TAIL) {
        const double nz = sqrt(tv / (2.0 * M) / (double)(H - kc));
        if (q > PP_TSTRIDE) { val = nz; dst = a.noise + rc; }
    }
    typedef double __attribute__((address_space(1)))* gdp_t;
    *(gdp_t)(uintptr_t)dst = val;
  } else {
    if ((tid & 3) == 0) {
        const int q = wave_reduce16_index(tid);
        if (q < PP_TSTRIDE) {
            // Re(i^q z): +Re, -Im, -Re, +Im, ...   (x 1/2: unhalved template against 2 d_k)
            tv *= 0.5;
            a.tay[tay_idx(rc, q)] = (q <= PP_TJ && ((q & 3) == 1 || (q & 3) == 2)) ? -tv : tv;
        }
    }
    if (tid == 4 * PP_TSTRIDE) a.sdraw[rc] = tv;
    if (TAIL && tid == 4 * (PP_TSTRIDE + 1)) a.noise[rc] = sqrt(tv / (2.0 * M) / (double)(H - kc));
  }
}

// The first row is waited for in front of the row loop, with a wait the compiler knows (vmcnt(0), the other counters
// left alone).  Its count at the top of a row has to hold on every way into the loop: coming from the kernel's start the
// row's last load was the youngest access in flight, coming from the previous row there is one younger, the result
// store -- so the top of EVERY row waited for vmcnt(0), the acknowledgement of a store issued a few instructions
// earlier.  With nothing in flight on entry the wait at the top is vmcnt(1): the row's data, and the store stays under way.
__device__ __forceinline__ void first_row_landed() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// Where the next row's loads are queued (measured choices, profiles/README.md): f64 rows in two
// halves -- eight registers' worth after the stage-1 twiddles (fftq1024's WHEN = 1), the rest
// behind the partner exchange -- and with the stage twiddles not held through the row (read back
// where they are used, see TWL in k_xspec_q1024); f32 rows whole, a quarter into stage 1
// (WHEN = 0), twiddles held.
constexpr int Q_PREFETCH_F64 = 1, Q_PREFETCH_F32 = 0;
// TAIL: also measure the noise from the top quarter of the power spectrum (errs == NULL,
// get_noise_PS): harmonics 768..1023 are this lane's registers 12..15 against the
// partner's registers 3..0 (five more registers published, four more read back), the
// Nyquist harmonic is Re Z_0 - Im Z_0.
template <typename Tin, bool TAIL>
__global__ __launch_bounds__(64, 2) void k_xspec_q1024(XspecArgs a) {
    constexpr int M = 1024, T = 64, R1 = 16, PER1 = 1;
    constexpr int NSL = 7;                     // slots: 2 Kt < M  ->  k <= 448 = 64 * 7
    typedef typename RawOf<Tin>::type Raw;
    constexpr int NRED = PP_TSTRIDE + (TAIL ? 2 : 1);       // the 12 Taylor sums, S_d (and the noise tail)
    static_assert(NRED <= 16, "wave_reduce_lds takes 16 values");
    constexpr int WRED = PP_WRED_DOUBLES(NRED) / 2;   // in cplx
    constexpr int LDSN = WRED > FFTQ_LDS_ELEMS ? WRED : FFTQ_LDS_ELEMS;
    static_assert(2 * LDSN >= PP_TAIL_LDS_DOUBLES, "tail_work's layout of this kernel's LDS");
    // TAIL, f64 rows: the template values of the last NML slots live in LDS beside the image instead of in registers
    // (with them held the kernel spilled one of them + three dwords to scratch, and the scratch reload in the middle
    // of the row queues behind the prefetched half row: vector memory returns in order).  The noise-given kernel does
    // not spill and keeps them in registers.
    constexpr bool F64 = sizeof(Tin) == 8;
    constexpr int NML = (F64 && TAIL) ? 2 : 0;
    // f64 rows, noise given: the lane's constants (stage twiddles t1, t2, split twiddle wb0) live in the wave's own LDS
    // and are read back, per row, where they are first used (TWL).  t2 (16 distinct values) takes free elements of the
    // transpose image; t1 and wb0 take two tables of 64 beside it (eight workgroups per CU: 8 x 19 456 B of the CU's
    // 160 KB -- at seven the kernel loses more than any wait costs).  With the noise measured the template slots have
    // taken that room and the three stay vector loads at the top of the row (TWR): t2 alone in LDS loses 0.2 - 0.3 %
    // (profiles/r07_lane_consts_ab.txt).
    constexpr bool TWL = F64 && !TAIL, TWR = F64 && TAIL;
    // phi_n through the scalar cache, one result store, the first row waited for in front of the loop
    constexpr bool ROWTOP = !TAIL;
    constexpr int NTW = TWL ? 2 : 0;
    __shared__ cplx lds[LDSN + 64 * (NML + NTW)];
    static_assert(sizeof(lds) <= 19456, "eight workgroups per CU");
    static_assert(FFTQ_FREE_ELEM0 + 15 * FFTQ_FREE_PITCH < FFTQ_LDS_ELEMS && FFTQ_FREE_ELEM0 >= 64 * (TAIL ? 12 : 7) &&
                  2 * FFTQ_FREE_ELEM0 >= PP_WRED_DOUBLES(NRED), "t2's elements are outside everything a row writes");
    cplx* const ldsm = lds + LDSN + threadIdx.x;
    int tid = threadIdx.x;
    const long long nrows = (long long)a.nsub * a.nchan;
    Raw cur[PER1][R1];
    // stage twiddles: W_1024^tid, W_64^(tid & 15)
    // f64 rows do not hold them (12 registers) through the whole row: with them held, three of the
    // template values spill to scratch, and a scratch reload queues BEHIND the prefetched
    // row (vector memory returns in order) -- the split then waits for the next row's HBM
    // data (15.1 -> 14.1 ms per 1024 fits).  TWL: the wave writes the three values to its own LDS once (and again after
    // tail_work, which uses the whole LDS) and the row reads them back with ds_read_b128 where they are used -- LDS
    // returns on lgkmcnt, not through the vector-memory queue, where an L1-resident load comes back behind every row
    // piece the CU's other seven waves have queued --; phi_n, one word for the whole wave, comes through the scalar
    // cache (k_setup / k_phase0 wrote it in an earlier launch; the tickets this launch carries belong to another work
    // set).  The row loop's vector memory is then the row stream, one result store and the per-chunk / per-channel
    // reads, and nothing else.  Worth 0.3 % by itself (profiles/r07_row_wait_ceiling.txt): the wait at the top of a
    // row is for the row.
    cplx t1 = a.twB[2 * tid], t2 = a.twB[32 * (tid & 15)];
    // this lane's harmonics k = kb + 64 j; split twiddle W_B^kb, stepped by W_B^64
    const int lam0 = fftq_lambda(tid);
    cplx wb0 = a.twB[lam0 ? lam0 : 64];
    const cplx wbT = a.twB[64];
    cplx* const ldt2 = lds + FFTQ_FREE_ELEM0;          // [17 (tid & 15)]
    cplx* const ldtw = lds + LDSN + 64 * NML;          // t1 [tid] | wb0 [64 + tid]
    auto put_lane_consts = [&](const cplx p1, const cplx p2, const cplx pb) {
        if (!TWL) return;
        ldt2[FFTQ_FREE_PITCH * (tid & 15)] = p2;       // (four lanes, the same value)
        ldtw[tid] = p1;
        ldtw[64 + tid] = pb;
        lds_sync<T>();
    };
    put_lane_consts(t1, t2, wb0);
    // (the previous batch's solve + post-fit stage, see tail_work: this wave draws ONE ticket after tail_after rows --
    // a different count for every wave, spread over the first three quarters of its share, so that at any time a
    // few per cent of the waves are out of the transform instead of half of them for the first millisecond --
    // and whatever is left once it has run out of rows)
    int tail_after = 0x7fffffff;
    if (a.tail) tail_after = ticket_moment(nrows);
    RowWalk<true> rw;
    rw.start(nrows, a.mwords, a.ticket, a.ticket_base);
    long long row = rw.row;
    int n = 0, i = 0;
    if (rw.more) {
        n = __builtin_amdgcn_readfirstlane((int)(row / a.nsub));
        i = __builtin_amdgcn_readfirstlane((int)(row % a.nsub));
        const size_t rc = (size_t)sub_of(a.act, i) * a.nchan_full + (a.coff + n * a.cstep);
        stage_load_global<M, T, R1>(cur, reinterpret_cast<const Tin*>(a.data) + rc * (2 * M), tid);
    }
    // this lane's template values (unhalved: the sums are halved at the end), reloaded
    // when the channel changes
    cplx mv2[NSL];
    const cplx* mheld = nullptr;
    const cplx* mrow = nullptr;    // the template row and cut of the channel in hand (channel_lookup)
    int n_held = -1, ktn = 0;
    int i_nx = i, n_nx = n;
    // FASTROW (f64 rows, noise given): the rows of a FULL chunk of one channel, walked without a mask, an `act` list or
    // per-subint templates, differ from their predecessor by one subint -- row, ph0 and result addresses advance by
    // nchan_full -- and none of them but the first draws a ticket or looks a channel up.  The chunk's first row (which
    // sees all that) counts them out, rows 1..30 take the short row top, and the last row is a general one again: it is
    // the one that moves on to the chunk the ticket names.  At two waves per SIMD a scalar or branch instruction takes
    // an issue slot of its wave that only the partner wave can fill: the general top walks ~80 of them a row.
    constexpr bool FASTROW = TWL;
    if (ROWTOP) first_row_landed();
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
    if (phase == 1) {
        if (!a.tail) break;
        // (between two rows: the next row's loads are in flight, the call keeps what it must across itself)
        tail_work(a.tail, reinterpret_cast<double*>(lds), 2 * (LDSN + 64 * NML), tid, 1);
        tail_after = 0x7fffffff;
        if (TWL) {      // (its layout covers the image: the lane constants again)
            const int lamr = fftq_lambda(tid);
            put_lane_consts(as_global(a.twB)[2 * tid], as_global(a.twB)[32 * (tid & 15)], as_global(a.twB)[lamr ? lamr : 64]);
        }
    }
    // (the short tops still to come in this chunk and the row they step from: values of THIS loop only -- the loop's
    // exit test is not wave-uniform to the compiler, and what it carries out of the loop lives in vector registers.
    // The walk is kept whole, so a wave back from tail_work finishes its chunk with general rows)
    unsigned fast_left = 0u;
    size_t rc_prev = 0;
    // (TWL: what a row needs of lambda -- kb and the partner's place in the published image -- in one register carried
    // across the rows, bits 0..9 the byte offset 16 fftq_lane_of((64 - lambda) & 63), bits 10..16 kb: two
    // instructions a row to unpack against fourteen to derive them from the lane number.  lambda = 0 is lane 0.)
    unsigned lanepk = 0u;
    if (TWL) {
        const int lamp = fftq_lambda(tid);
        lanepk = 16u * (unsigned)fftq_lane_of((64 - lamp) & 63) | (unsigned)(lamp ? lamp : 64) << 10;
    }
    for (; rw.more && tail_after != 0; rw.advance(), row = rw.row, i = i_nx, n = n_nx, --tail_after) {
        // (FASTROW: the walk's steps sit in the general branch of the row top below.  The kernels without it keep
        // theirs where they were measured)
        if (!FASTROW) {
            rw.draw(a.ticket);
            rw.peek(nrows, a.ticket_base, a.mwords);
        }
        // (what is derived from the lane number is recomputed per row: held across the row it would cost the
        // registers the prefetched row needs -- all but TWL's one packed word, lanepk)
        asm volatile("" : "+v"(tid));
        if (TWL) {
            asm volatile("" : "+v"(lanepk));
            __builtin_assume((unsigned)tid < 64u);      // (behind the barrier the compiler has forgotten it: masks, range tests)
        }
        const int lam = TWL ? 0 : fftq_lambda(tid);       // (TWL: not used)
        const bool l0 = TWL ? (tid == 0) : (lam == 0);
        const int kb = TWL ? (int)(lanepk >> 10) : (l0 ? 64 : lam);
        if (TWR) {
            t1 = as_global(a.twB)[2 * tid];
            t2 = as_global(a.twB)[32 * (tid & 15)];
            wb0 = as_global(a.twB)[kb];
        } else if (!TWL) {      // (TWL: read where they are used)
            asm volatile("" : "+v"(t1.x), "+v"(t1.y), "+v"(t2.x), "+v"(t2.y), "+v"(wb0.x), "+v"(wb0.y));
        }
        size_t rc;
        const Tin* nxrow = nullptr;
        if (FASTROW && fast_left != 0u) {
            // one subint on in the same chunk and channel: no ticket, no mask word, no look-up; the row after it too
            --fast_left;
            rc = rc_prev + (size_t)(unsigned)a.nchan_full;
            rw.row_nx = rw.row + 1u;
            rw.bits &= rw.bits - 1u;
            i_nx = i + 1;
            nxrow = reinterpret_cast<const Tin*>(a.data) + (rc + (size_t)(unsigned)a.nchan_full) * (2 * M);
        } else {
            if (FASTROW) {
                rw.draw(a.ticket);
                rw.peek(nrows, a.ticket_base, a.mwords);
            }
            const int ia = sub_of(a.act, i), ne = a.coff + n * a.cstep;   // true subint, channel
            rc = (size_t)ia * a.nchan_full + ne;
            // loads whose results are needed late are issued before the prefetch (vector
            // memory returns in order)
            if (channel_lookup(a, ia, n, ne, M, n_held, mrow, ktn) && mrow != mheld) {
#pragma unroll
                for (int j = 0; j < NSL; ++j) {
                    const cplx mval = mrow[kb + 64 * j - 1];   // k <= 448: inside the row
                    if (j < NSL - NML) mv2[j] = mval; else ldsm[64 * (j - (NSL - NML))] = mval;
                }
                mheld = mrow;
            }
            if (FASTROW) {
                const bool first_of_chunk = rw.fresh != 0u;
                rw.next(i, n, i_nx, n_nx, nrows, a.nsub, a.ticket_base, a.ticket, a.mwords);
                nxrow = next_row_of<M, Tin>(a, rw.more_nx, i_nx, n_nx, rc);
                // a full chunk (rows 2..31 still to come behind the next one) of one channel, every row in use
                const bool whole = first_of_chunk && rw.bits == 0xfffffffcu && i + (PP_ROW_CHUNK - 1) < a.nsub &&
                                   !a.mwords && !a.act && !a.slot;
                // (a scalar register: the count is tested and stepped at the top of every row)
                fast_left = (unsigned)__builtin_amdgcn_readfirstlane(whole ? PP_ROW_CHUNK - 2 : 0);
            }
        }
        rc_prev = rc;
        const double phin = ROWTOP ? load_uniform(a.ph0 + rc) : a.ph0[rc];
        double sd = 0.0;
        cplx v[R1];
#pragma unroll
        for (int k = 0; k < R1; ++k) v[k] = to_cplx(cur[0][k]);
        // the next row's HBM loads are queued as soon as this row's registers are dead
        // (unconditional: the last row of the run fetches itself again, see k_xspec)
        // f64 rows: in two halves -- eight registers' worth inside the first stage, the
        // rest once the second half of this row's outputs has been published: with the
        // whole next row in flight from the start, 64 + 64 row registers on top of the
        // template row and the sums do not fit the 256 of two waves per SIMD
        constexpr bool HALVES = F64;
        // (pieces k0 .. k1 - 1 of the next row.  A lambda over the kernel's own variables in every kernel that queues a
        // row in pieces, not a direct call: k_xspec_qf<1024> keeps three more scalar registers alive across its call
        // to tail_work with the direct call -- profiles/r08_refactor_isa.txt)
        auto load_some = [&](int k0, int k1) { load_row_pieces<Raw, R1, FASTROW>(cur, nxrow, tid, k0, k1); };
        // (the row after this one is decided HERE or in the row top, outside the lambda: a walk captured by reference
        // is not split into registers -- its flags went through scratch memory, whose loads queue behind the
        // prefetched row -- and at the top of a row everything older than this row's own data has landed,
        // the ticket of the chunk's first row included)
        if (!FASTROW) {
            rw.next(i, n, i_nx, n_nx, nrows, a.nsub, a.ticket_base, a.ticket, a.mwords);
            nxrow = next_row_of<M, Tin>(a, rw.more_nx, i_nx, n_nx, rc);
        }
        auto prefetch = [&]() {
            __builtin_amdgcn_sched_barrier(0);
            load_some(0, HALVES ? R1 / 2 : R1);
            __builtin_amdgcn_sched_barrier(0);
        };
        fftq1024_from<(sizeof(Tin) == 8 ? Q_PREFETCH_F64 : Q_PREFETCH_F32), TWL>(
            v, lds, [&]() { return NTW ? ldtw[tid] : t1; }, [&]() { return TWL ? ldt2[FFTQ_FREE_PITCH * (tid & 15)] : t2; },
            tid, &sd, prefetch);
        __builtin_amdgcn_sched_barrier(0);
        // ---- partners through LDS: registers 9..15 out, seven values back ----
        {
            cplx* pub = lds + tid;
#pragma unroll
            for (int r = 0; r < NSL; ++r) pub[64 * r] = v[9 + r];
            if (TAIL) {
#pragma unroll
                for (int r = 0; r < 5; ++r) pub[64 * (NSL + r)] = v[r];
            }
            lds_sync<T>();
        }
        if (NTW) wb0 = ldtw[64 + tid];
        double tail = 0.0;
        if (TAIL) {
            // |2 d_k|^2 for k = lam + 64 kd, kd = 12..15; W_B^k = W_B^kb0 W_B^(64 kd) with
            // kb0 = lam (the lane that owns lam = 0: kb = 64, one step ahead) and
            // W_B^768 = exp(-3 pi i / 4).  Partner: register 15 - kd of the partner lane
            // (own register 16 - kd for lam = 0).
            const double h = 0.70710678118654752440;
            const cplx* pt = lds + fftq_lane_of((64 - lam) & 63) + (l0 ? 64 : 0);
            // lam != 0: W^lam W^768;  lam = 0: wb0 = W^64, wanted W^768 = W^64 W^704 -> use W^768 directly
            cplx wt = l0 ? make_double2(-h, -h) : cmul(wb0, make_double2(-h, -h));
#pragma unroll
            for (int kd = 12; kd < 16; ++kd) {
                tail += cnorm(split_pair(v[kd], pt[64 * (NSL + 15 - kd)], wt));
                wt = cmul(wt, wbT);
            }
            tail *= 0.25;
            if (tid == 0) { const double dM = v[0].x - v[0].y; tail += dM * dM; }
        }
        if (HALVES) {
            __builtin_amdgcn_sched_barrier(0);
            load_some(R1 / 2, R1);
            __builtin_amdgcn_sched_barrier(0);
        }
        // slot j: register 15 - j -> pc[64 (6 - j)]
        const cplx* pc = TWL ? reinterpret_cast<const cplx*>(reinterpret_cast<const char*>(lds) + (lanepk & 0x3ffu))
                             : lds + fftq_lane_of((64 - lam) & 63);
        // ---- phasors: e^{2 pi i kb phi}; lane 0 (kb = 64) holds the step ----
        const cplx el = unit_phasor<true, TWL>((double)kb, phin);
        const cplx wst = make_double2(bcast_lane0(el.x), bcast_lane0(el.y));
        cplx e = el, wb = wb0;
        const int ktu = __builtin_amdgcn_readfirstlane(ktn);
        const double kap0 = PP_TWO_PI * (double)kb;
        double tm[PP_TSTRIDE];
        // (the partner value of the slot in hand and of the next one: TWL alternates between two registers' worth --
        // carried in one variable the hand-over is two v_mov_b64 a slot)
        cplx zq[2];
        zq[0] = pc[64 * 6];
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            if (j > 0 && !(64 * j < ktu)) break;     // (kept slots are a prefix)
            const cplx zc = zq[TWL ? (j & 1) : 0];
            if (j + 1 < NSL && 64 * (j + 1) < ktu) zq[TWL ? ((j + 1) & 1) : 0] = pc[64 * (5 - j)];
            // the template cut is a multiple of 64: a slot is kept or dropped as a whole
            if (j == 0 || 64 * j < ktu) {
                const cplx dd = split_pair(csel(l0, v[j + 1], v[j]), zc, wb);
                const cplx mj = (j < NSL - NML) ? mv2[j < NSL - NML ? j : 0] : ldsm[64 * (j - (NSL - NML))];
                const cplx x = cmulc(dd, mj);
                const cplx z = cmul(x, e);
                const double kap = j == 0 ? kap0 : kap0 + kconst<true>(PP_TWO_PI * (double)(64 * j));
                taylor_terms(j == 0, tm, x, z, kap);
            }
            if (j + 1 < NSL && 64 * (j + 1) < ktu) {
                wb = cmul(wb, wbT);
                e = cmul(e, wst);
            }
        }
        // ---- the 12 sums and S_d: one reduction through LDS ----
        double tr[NRED];
#pragma unroll
        for (int j = 0; j < PP_TSTRIDE; ++j) tr[j] = tm[j];
        tr[PP_TSTRIDE] = sd;
        if (TAIL) tr[NRED - 1] = tail;
        lds_sync<T>();      // (the partner reads are older than the reduction's writes)
        double tv = wave_reduce_lds<NRED, TWL>(tr, tid, reinterpret_cast<double*>(lds));
        store_row_results<M, TAIL, ROWTOP, TWL>(a, rc, tid, tv);
        lds_sync<T>();
    }
    }
    // (out of rows: the tickets of the previous batch's tail that are left)
    if (a.tail) tail_work(a.tail, reinterpret_cast<double*>(lds), 2 * (LDSN + 64 * NML), tid, 1 << 30);
}


// --------------------------------------------------------------------------
// The same for templates that keep 512 harmonics or more (k_xspec's MODE 3; data-derived
// spline / PCA templates keep all 1024): every lane works on all 16 of its harmonics
// k = kb + 64 j, publishes all 16 registers and reads 16 partner values.  The lane that
// owns lam = 0 takes k = 64 (j + 1) from register (j + 1) & 15 -- its slot 15 is the Nyquist
// harmonic, for which the general split formula with Z_k = Z_{M-k} = Z_0 and W_B^M = -1
// gives 2 (Re Z_0 - Im Z_0) --, so one wave-uniform test keeps or drops a slot for every lane.
// The 16 template values of a lane (64 registers) cannot live beside two rows: they are
// read every row (L2 hits) between the transpose and the last stage, and the next row's
// loads are queued only after them, at the start of the split, in two halves (vector memory
// returns in order: template reads issued after the prefetch would wait for HBM).
// --------------------------------------------------------------------------
// TAIL (errs == NULL): harmonics 768..1024 are slots 12..15 (11..15 for the lane that owns
// lam = 0, whose slot 15 is the Nyquist harmonic); their split is formed whether or not the
// template keeps them.
// M = 512 (1024-bin rows, plan 8.4.2.8 of pp_fftq.h): the same with 8 harmonics per lane; serves every
// template cut (slots beyond it are skipped) -- configs[1]'s template keeps 448 of 512 harmonics.
// k_xspec_qf, 2048-bin rows with the noise given: phi_n through the scalar cache, the row's results in one store, the
// first row waited for in front of the loop (QTOP; see store_row_results, first_row_landed): +0.5 %.  Not the others:
// -0.6 % for 1024-bin rows (three waves per SIMD hide the wait already) and -0.3 % for 2048-bin rows whose noise is
// measured (as in k_xspec_q1024; profiles/r07_lane_consts_ab.txt).  The stage twiddles stay where they are (Q::run)
constexpr int PP_QF512_WPS = 3;      // waves per SIMD the 1024-bin kernel is compiled for
template <int M, typename Tin, bool TAIL>
__global__ __launch_bounds__(64, (M == 1024 ? 2 : PP_QF512_WPS)) void k_xspec_qf(XspecArgs a) {
    typedef FftQ<M> Q;
    constexpr int T = 64, R1 = Q::R, PER1 = 1;
    constexpr int NSL = R1;
    constexpr int JT = (3 * NSL) / 4;        // first slot of the noise tail (k >= int(0.75 (M + 1)) = 64 JT)
    static_assert((int)(0.75 * (M + 1)) == 64 * JT, "the noise tail starts on a slot boundary");
    typedef typename RawOf<Tin>::type Raw;
    constexpr int NRED = PP_TSTRIDE + (TAIL ? 2 : 1);       // the 12 Taylor sums, S_d (and the noise tail)
    constexpr int WRED = PP_WRED_DOUBLES(NRED) / 2;   // in cplx
    constexpr int LDSN0 = Q::LDS_ELEMS > 64 * NSL ? Q::LDS_ELEMS : 64 * NSL;     // transpose image | published registers
    constexpr int LDSN = WRED > LDSN0 ? WRED : LDSN0;
    static_assert(M != 1024 || 2 * LDSN >= PP_TAIL_LDS_DOUBLES, "tail_work's layout of this kernel's LDS");
    __shared__ cplx lds[LDSN];
    int tid = threadIdx.x;
    constexpr bool QTOP = M == 1024 && !TAIL;
    const long long nrows = (long long)a.nsub * a.nchan;
    Raw cur[PER1][R1];
    const cplx wbT = a.twB[64];
    // (tickets as in k_xspec_q1024, for 2048-bin rows only: the 1024-bin kernel is compiled for three waves per SIMD, 168
    // registers, and a function called from it inherits that budget -- tail_work then spills, in every carrier:
    // configs[1] lost 6 % with it)
    int tail_after = 0x7fffffff;
    if (M == 1024 && a.tail) tail_after = ticket_moment(nrows);
    RowWalk<true> rw;
    rw.start(nrows, a.mwords, a.ticket, a.ticket_base);
    long long row = rw.row;
    int n = 0, i = 0;
    if (rw.more) {
        n = __builtin_amdgcn_readfirstlane((int)(row / a.nsub));
        i = __builtin_amdgcn_readfirstlane((int)(row % a.nsub));
        const size_t rc = (size_t)sub_of(a.act, i) * a.nchan_full + (a.coff + n * a.cstep);
        stage_load_global<M, T, R1>(cur, reinterpret_cast<const Tin*>(a.data) + rc * (2 * M), tid);
    }
    int i_nx = i, n_nx = n;
    const cplx* mrow = nullptr;    // the template row and cut of the channel in hand (channel_lookup)
    int n_held = -1, ktn = 0;
    // 1024-bin rows: the lane's 8 template values are HELD while the channel does not change (32 registers; the 16
    // values of a 2048-bin row's lane do not fit beside two rows and are read every row)
    constexpr bool MHOLD = M == 512;
    cplx mv[NSL];
    const cplx* mheld = nullptr;
    if (QTOP) first_row_landed();
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
    if (phase == 1) {
        if (!(M == 1024 && a.tail)) break;
        tail_work(a.tail, reinterpret_cast<double*>(lds), 2 * LDSN, tid, 1);
        tail_after = 0x7fffffff;
    }
    for (; rw.more && tail_after != 0; rw.advance(), row = rw.row, i = i_nx, n = n_nx, --tail_after) {
        rw.draw(a.ticket);
        rw.peek(nrows, a.ticket_base, a.mwords);
        asm volatile("" : "+v"(tid));
        const int lam = Q::lambda(tid);
        const bool l0 = (lam == 0);
        const int kb = l0 ? 64 : lam;
        const cplx wb0 = as_global(a.twB)[kb];
        const int ia = sub_of(a.act, i), ne = a.coff + n * a.cstep;   // true subint, channel
        const size_t rc = (size_t)ia * a.nchan_full + ne;
        const bool looked = channel_lookup(a, ia, n, ne, M, n_held, mrow, ktn);
        if (MHOLD && looked && mrow != mheld) {
#pragma unroll
            for (int j = 0; j < NSL; ++j) mv[j] = mrow[kb + 64 * j - 1];
            mheld = mrow;
        }
        const double phin = QTOP ? load_uniform(a.ph0 + rc) : a.ph0[rc];
        double sd = 0.0;
        cplx v[R1];
#pragma unroll
        for (int k = 0; k < R1; ++k) v[k] = to_cplx(cur[0][k]);
        // this lane's 16 template values, read between the transpose and the last stage
        auto template_loads = [&]() {
            if (MHOLD) return;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NSL; ++j) mv[j] = mrow[kb + 64 * j - 1];   // k <= 1024: inside the row
            __builtin_amdgcn_sched_barrier(0);
        };
        Q::template run<3>(v, lds, as_global(a.twB), tid, &sd, template_loads);
        __builtin_amdgcn_sched_barrier(0);
        // ---- partners through LDS: all 16 registers out, 16 values back ----
        {
            cplx* pub = lds + tid;
#pragma unroll
            for (int s = 0; s < NSL; ++s) pub[64 * s] = v[s];
            lds_sync<T>();
        }
        // ---- the next row: first half now (behind the template reads), second half after slot 7 ----
        const Tin* nxrow;
        auto load_some = [&](int k0, int k1) { load_row_pieces<Raw>(cur, nxrow, tid, k0, k1); };
        {
            __builtin_amdgcn_sched_barrier(0);
            rw.next(i, n, i_nx, n_nx, nrows, a.nsub, a.ticket_base, a.ticket, a.mwords);
            nxrow = next_row_of<M, Tin>(a, rw.more_nx, i_nx, n_nx, rc);
            load_some(0, R1 / 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        const cplx* pc = lds + Q::lane_of((64 - lam) & 63);   // slot j: register NSL - 1 - j of the partner
        const cplx el = unit_phasor<true>((double)kb, phin);
        const cplx wst = make_double2(bcast_lane0(el.x), bcast_lane0(el.y));
        cplx e = el, wb = wb0;
        const int ktu = __builtin_amdgcn_readfirstlane(ktn);
        const double kap0 = PP_TWO_PI * (double)kb;
        double tm[PP_TSTRIDE];
        double tail = 0.0;
        cplx zc_nx = pc[64 * (NSL - 1)];
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            // (noise given: the kept slots are a prefix and nothing beyond them is needed.  The loop may only END once
            // the second half of the next row's loads has been queued, at slot NSL / 2 -- a copy of those loads at
            // every earlier exit cost the kernel its register allocation: 54 / 123 spilled VGPRs --; before that a
            // dropped slot just skips its body, its recurrences and its partner read)
            if (!TAIL && j > NSL / 2 && !(64 * j < ktu)) break;
            const cplx zc = zc_nx;
            if (j + 1 < NSL && (TAIL || 64 * (j + 1) < ktu)) zc_nx = pc[64 * (NSL - 2 - j)];
            if (j == NSL / 2) {
                __builtin_amdgcn_sched_barrier(0);
                load_some(R1 / 2, R1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the template cut is a multiple of 64: a slot is kept or dropped as a whole
            const bool keep = (j == 0 || 64 * j < ktu);
            if (keep || (TAIL && j >= JT - 1)) {
                const cplx dd = split_pair(csel(l0, v[(j + 1) & (NSL - 1)], v[j]), zc, wb);
                if (TAIL && j >= JT - 1) {
                    const double pw = cnorm(dd);
                    tail += (j >= JT || l0) ? pw : 0.0;
                }
              if (keep) {
                const cplx x = cmulc(dd, mv[j]);
                const cplx z = cmul(x, e);
                const double kap = j == 0 ? kap0 : kap0 + kconst<true>(PP_TWO_PI * (double)(64 * j));
                taylor_terms(j == 0, tm, x, z, kap);
              }
            }
            if (TAIL || (j + 1 < NSL && 64 * (j + 1) < ktu)) {
                wb = cmul(wb, wbT);
                e = cmul(e, wst);
            }
        }
        double tr[NRED];
#pragma unroll
        for (int j = 0; j < PP_TSTRIDE; ++j) tr[j] = tm[j];
        tr[PP_TSTRIDE] = sd;
        if (TAIL) tr[NRED - 1] = 0.25 * tail;
        lds_sync<T>();      // (the partner reads are older than the reduction's writes)
        double tv = wave_reduce_lds(tr, tid, reinterpret_cast<double*>(lds));
        store_row_results<M, TAIL, QTOP>(a, rc, tid, tv);
        lds_sync<T>();
    }
    }
    if (M == 1024 && a.tail) tail_work(a.tail, reinterpret_cast<double*>(lds), 2 * LDSN, tid, 1 << 30);
}

}  // namespace pp
