// k_xspec_cu1024: k_xspec_q1024<double, false> (pp_xspec1024q.h: 2048-bin f64 rows, noise given, template cut below
// 512 harmonics) with the CU's eight waves in ONE workgroup, so that what a row computes from the lane number alone is
// computed once per launch and shared.
//
// Two pieces of a row's f64 work have operands that do not depend on the row: the powers t1^2 .. t1^15 of the lane's
// stage-1 twiddle (fftq1024_from's product tree) and the steps wb0 wbT^j of its split twiddle (the slot loop's
// cmul(wb, wbT)).  A table of (power, lane) is the same for every wave: 15 KB + 7 KB.  Eight one-wave workgroups have
// 19 456 B each and no room for it; one workgroup of eight waves has
//
//   8 x 17 408 B  the waves' transpose images, each a wave's own (base wave * 17 408; t2 in its free elements)
//   15 x 1 024 B  T1[j - 1][lane] = t1^j, j = 1 .. 15
//    7 x 1 024 B  WB[j][lane] = wb0 wbT^j, j = 0 .. 6                                  161 792 B of 163 840
//
// Wave 0 fills the tables at the start with the operations, in the order, the row did: every entry has the bits
// k_xspec_q1024 computes, and so has everything downstream.  ONE barrier follows the fill, which every thread reaches;
// after it no wave waits for another -- a wave is what a workgroup of k_xspec_q1024 is (RowWalk's and ticket_moment's
// CU flag: number 8 blockIdx.x + wave of 8 gridDim.x), draws its chunks and tickets as one, and leaves when it is done.
// A ticket (tail_work_wave) uses the wave's image alone and its barriers are the wave's own (team_sync); the tables
// lie outside every image and are never written again.
//
// The row is k_xspec_q1024's TWL path line by line, apart from where the three values come from.  The kernel is
// compiled in a translation unit of its own (pp_xspec_cu.hip says why); the host reaches it through that unit's two
// functions.
#pragma once
#include "pp_xspec1024q.h"

namespace pp {

constexpr int CU_WAVES = 8, CU_NT1 = 15, CU_NWB = 7;
constexpr int CU_IMAGE_ELEMS = FFTQ_LDS_ELEMS;                                         // per wave, in cplx
constexpr int CU_LDS_BYTES = (CU_WAVES * CU_IMAGE_ELEMS + 64 * (CU_NT1 + CU_NWB)) * (int)sizeof(cplx);
static_assert(CU_LDS_BYTES == 161792 && CU_LDS_BYTES <= 163840, "one workgroup per CU, the whole LDS");
static_assert(2 * CU_IMAGE_ELEMS >= PP_TAIL_LDS_DOUBLES, "tail_work's layout of a wave's image");

template <typename Tin>
__global__ __launch_bounds__(64 * CU_WAVES, 2) void k_xspec_cu1024(XspecArgs a) {
    constexpr int M = 1024, T = 64, R1 = 16, PER1 = 1;
    constexpr int NSL = CU_NWB;                // slots: 2 Kt < M  ->  k <= 448 = 64 * 7
    typedef typename RawOf<Tin>::type Raw;
    static_assert(sizeof(Tin) == 8, "f64 rows");
    constexpr int NRED = PP_TSTRIDE + 1;       // the 12 Taylor sums, S_d
    constexpr int LDSN = CU_IMAGE_ELEMS;
    static_assert(PP_WRED_DOUBLES(NRED) / 2 <= LDSN, "the reduction inside the image");
    static_assert(FFTQ_FREE_ELEM0 + 15 * FFTQ_FREE_PITCH < FFTQ_LDS_ELEMS && FFTQ_FREE_ELEM0 >= 64 * 7 &&
                  2 * FFTQ_FREE_ELEM0 >= PP_WRED_DOUBLES(NRED), "t2's elements are outside everything a row writes");
    extern __shared__ cplx cu_lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int tid = threadIdx.x & 63;
    cplx* const lds = cu_lds + wave * LDSN;                       // this wave's image
    cplx* const tab1 = cu_lds + CU_WAVES * LDSN;                  // T1[j - 1][lane]
    cplx* const tabw = tab1 + 64 * CU_NT1;                        // WB[j][lane]
    const long long nrows = (long long)a.nsub * a.nchan;
    Raw cur[PER1][R1];
    if (wave == 0) {
        // the product tree of fftq1024_from and the slot loop's steps, operation by operation
        cplx wq[16];
        wq[1] = a.twB[2 * tid];
#pragma unroll
        for (int j = 2; j < 16; ++j) {
            if (j % 2 == 0) {
                const cplx h = wq[j / 2];
                wq[j] = make_double2(fma(h.x, h.x, -h.y * h.y), 2.0 * h.x * h.y);
            } else wq[j] = cmul(wq[j - 1], wq[1]);
        }
#pragma unroll
        for (int j = 1; j < 16; ++j) tab1[64 * (j - 1) + tid] = wq[j];
        const int lamf = fftq_lambda(tid);
        cplx wb = a.twB[lamf ? lamf : 64];
        const cplx wbT = a.twB[64];
#pragma unroll
        for (int j = 0; j < CU_NWB; ++j) {
            tabw[64 * j + tid] = wb;
            wb = cmul(wb, wbT);
        }
    }
    cplx* const ldt2 = lds + FFTQ_FREE_ELEM0;          // [17 (tid & 15)]
    auto put_lane_consts = [&](const cplx p2) {
        ldt2[FFTQ_FREE_PITCH * (tid & 15)] = p2;       // (four lanes, the same value)
        lds_sync<T>();
    };
    put_lane_consts(a.twB[32 * (tid & 15)]);
    // (the one barrier of the kernel: in front of every exit, the tables are complete behind it)
    __syncthreads();
    int tail_after = 0x7fffffff;
    if (a.tail) tail_after = ticket_moment<true>(nrows);
    RowWalk<true, true> rw;
    rw.start(nrows, a.mwords, a.ticket, a.ticket_base);
    long long row = rw.row;
    int n = 0, i = 0;
    if (rw.more) {
        n = __builtin_amdgcn_readfirstlane((int)(row / a.nsub));
        i = __builtin_amdgcn_readfirstlane((int)(row % a.nsub));
        const size_t rc = (size_t)sub_of(a.act, i) * a.nchan_full + (a.coff + n * a.cstep);
        stage_load_global<M, T, R1>(cur, reinterpret_cast<const Tin*>(a.data) + rc * (2 * M), tid);
    }
    cplx mv2[NSL];
    const cplx* mheld = nullptr;
    const cplx* mrow = nullptr;    // the template row and cut of the channel in hand (channel_lookup)
    int n_held = -1, ktn = 0;
    int i_nx = i, n_nx = n;
    first_row_landed();
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
    if (phase == 1) {
        if (!a.tail) break;
        tail_work_wave(a.tail, reinterpret_cast<double*>(lds), 2 * LDSN, tid, 1);
        tail_after = 0x7fffffff;
        put_lane_consts(as_global(a.twB)[32 * (tid & 15)]);      // (its layout covers the image; the tables are outside)
    }
    unsigned fast_left = 0u;
    size_t rc_prev = 0;
    unsigned lanepk = 0u;
    {
        const int lamp = fftq_lambda(tid);
        lanepk = 16u * (unsigned)fftq_lane_of((64 - lamp) & 63) | (unsigned)(lamp ? lamp : 64) << 10;
    }
    for (; rw.more && tail_after != 0; rw.advance(), row = rw.row, i = i_nx, n = n_nx, --tail_after) {
        asm volatile("" : "+v"(tid));
        asm volatile("" : "+v"(lanepk));
        __builtin_assume((unsigned)tid < 64u);
        const bool l0 = (tid == 0);
        const int kb = (int)(lanepk >> 10);
        size_t rc;
        const Tin* nxrow = nullptr;
        if (fast_left != 0u) {
            // one subint on in the same chunk and channel: no ticket, no mask word, no look-up; the row after it too
            --fast_left;
            rc = rc_prev + (size_t)(unsigned)a.nchan_full;
            rw.row_nx = rw.row + 1u;
            rw.bits &= rw.bits - 1u;
            i_nx = i + 1;
            nxrow = reinterpret_cast<const Tin*>(a.data) + (rc + (size_t)(unsigned)a.nchan_full) * (2 * M);
        } else {
            rw.draw(a.ticket);
            rw.peek(nrows, a.ticket_base, a.mwords);
            const int ia = sub_of(a.act, i), ne = a.coff + n * a.cstep;   // true subint, channel
            rc = (size_t)ia * a.nchan_full + ne;
            if (channel_lookup(a, ia, n, ne, M, n_held, mrow, ktn) && mrow != mheld) {
#pragma unroll
                for (int j = 0; j < NSL; ++j) mv2[j] = mrow[kb + 64 * j - 1];   // k <= 448: inside the row
                mheld = mrow;
            }
            const bool first_of_chunk = rw.fresh != 0u;
            rw.next(i, n, i_nx, n_nx, nrows, a.nsub, a.ticket_base, a.ticket, a.mwords);
            nxrow = next_row_of<M, Tin>(a, rw.more_nx, i_nx, n_nx, rc);
            const bool whole = first_of_chunk && rw.bits == 0xfffffffcu && i + (PP_ROW_CHUNK - 1) < a.nsub &&
                               !a.mwords && !a.act && !a.slot;
            fast_left = (unsigned)__builtin_amdgcn_readfirstlane(whole ? PP_ROW_CHUNK - 2 : 0);
        }
        rc_prev = rc;
        const double phin = load_uniform(a.ph0 + rc);
        double sd = 0.0;
        cplx v[R1];
#pragma unroll
        for (int k = 0; k < R1; ++k) v[k] = to_cplx(cur[0][k]);
        auto load_some = [&](int k0, int k1) { load_row_pieces<Raw, R1, true>(cur, nxrow, tid, k0, k1); };
        auto prefetch = [&]() {
            __builtin_amdgcn_sched_barrier(0);
            load_some(0, R1 / 2);
            __builtin_amdgcn_sched_barrier(0);
        };
        fftq1024_from<Q_PREFETCH_F64, true, true>(
            v, lds, [&](const int j) { return tab1[64 * (j - 1) + tid]; }, [&]() { return ldt2[FFTQ_FREE_PITCH * (tid & 15)]; },
            tid, &sd, prefetch);
        __builtin_amdgcn_sched_barrier(0);
        // ---- partners through LDS: registers 9..15 out, seven values back ----
        {
            cplx* pub = lds + tid;
#pragma unroll
            for (int r = 0; r < NSL; ++r) pub[64 * r] = v[9 + r];
            lds_sync<T>();
        }
        // (the split twiddle of the slot in hand and of the next one, read a slot ahead like the partner value)
        cplx wbq[2];
        wbq[0] = tabw[tid];
        __builtin_amdgcn_sched_barrier(0);
        load_some(R1 / 2, R1);
        __builtin_amdgcn_sched_barrier(0);
        // slot j: register 15 - j -> pc[64 (6 - j)]
        const cplx* pc = reinterpret_cast<const cplx*>(reinterpret_cast<const char*>(lds) + (lanepk & 0x3ffu));
        // ---- phasors: e^{2 pi i kb phi}; lane 0 (kb = 64) holds the step ----
        const cplx el = unit_phasor<true, true>((double)kb, phin);
        const cplx wst = make_double2(bcast_lane0(el.x), bcast_lane0(el.y));
        cplx e = el;
        const int ktu = __builtin_amdgcn_readfirstlane(ktn);
        const double kap0 = PP_TWO_PI * (double)kb;
        double tm[PP_TSTRIDE];
        cplx zq[2];
        zq[0] = pc[64 * 6];
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            if (j > 0 && !(64 * j < ktu)) break;     // (kept slots are a prefix)
            const cplx zc = zq[j & 1];
            const cplx wb = wbq[j & 1];
            if (j + 1 < NSL && 64 * (j + 1) < ktu) {
                zq[(j + 1) & 1] = pc[64 * (5 - j)];
                wbq[(j + 1) & 1] = tabw[64 * (j + 1) + tid];     // (k_xspec_q1024: wb = cmul(wb, wbT))
            }
            if (j == 0 || 64 * j < ktu) {
                const cplx dd = split_pair(csel(l0, v[j + 1], v[j]), zc, wb);
                const cplx x = cmulc(dd, mv2[j]);
                const cplx z = cmul(x, e);
                const double kap = j == 0 ? kap0 : kap0 + kconst<true>(PP_TWO_PI * (double)(64 * j));
                taylor_terms(j == 0, tm, x, z, kap);
            }
            if (j + 1 < NSL && 64 * (j + 1) < ktu) e = cmul(e, wst);
        }
        // ---- the 12 sums and S_d: one reduction through LDS ----
        double tr[NRED];
#pragma unroll
        for (int j = 0; j < PP_TSTRIDE; ++j) tr[j] = tm[j];
        tr[PP_TSTRIDE] = sd;
        lds_sync<T>();      // (the partner reads are older than the reduction's writes)
        double tv = wave_reduce_lds<NRED, true>(tr, tid, reinterpret_cast<double*>(lds));
        store_row_results<M, false, true, true>(a, rc, tid, tv);
        lds_sync<T>();
    }
    }
    // (out of rows: the tickets of the previous batch's tail that are left)
    if (a.tail) tail_work_wave(a.tail, reinterpret_cast<double*>(lds), 2 * LDSN, tid, 1 << 30);
}

}  // namespace pp
