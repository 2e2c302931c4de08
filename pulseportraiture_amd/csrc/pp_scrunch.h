// Time, frequency and polarisation scrunching (what load_data hands to PSRCHIVE, pplib.py:2650-2814): one streaming
// pass over src[nsub][npol][nchan][nbin],
//   out[gt][p'][gf][b] = sum_{s in T_gt} sum_{c in F_gf} w[s][c] x[s][p][c][b] / sum_{s, c} w[s][c]
// No transform and no atomics: ONE thread owns 16 bytes' worth of input bins of one output row (four f32 or two f64
// samples -> four or two f64 sums) and adds that row's members in the order the host lists them -- ascending (subint,
// channel), rows of weight 0 or NaN left out, so their samples are never read.  The sum is a chain of f64 fma's and
// is divided once at the end: the bits of an output element depend on its own members only, not on the grid, on the
// other groups of the call or on how a host input is cut into runs (a time group that straddles two runs keeps its
// partial sums in `out` and goes on from them).
// The pass is bandwidth bound: a thread issues the loads of PP_SCRUNCH_UNROLL members before the first add, and small
// outputs are cut into one-wave workgroups so that they reach as many compute units as they have waves.
#pragma once

namespace pp {

#define PP_SCRUNCH_UNROLL 8     // member rows whose loads are in flight per thread

// one live member row of an output cell: its weight, and its row (s npol) nchan + c of the run's polarisation 0
struct ScrunchMember {
    double w;
    long long row;
};

struct ScrunchArgs {
    const void* src;            // the run's [n][npol][nchan][nbin]
    double* out;                // [ngt][npo][ngf][nbin] of the run's time groups
    const ScrunchMember* mem;   // the cells' member lists, cell (gt, gf) at off[gt ngf + gf] .. off[gt ngf + gf + 1]
    const int* off;
    const double* wtot;         // [ngt][ngf] total weight of the WHOLE group (all runs); not positive: a dead cell
    const int* tflag;           // [ngt] bit 0: `out` holds the group's partial sums of earlier runs; bit 1: it ends here
    int ngt, npo, ngf, nchan, nbin;
};

// N samples of a row by one load: 16 bytes where all of them are inside the row, 8 for the tail of an f32 row.  Rows
// have an even number of samples, so every row of an 8-byte aligned array starts on 8 bytes (not on 16: nbin = 102)
template <typename T, int N>
__device__ __forceinline__ void scrunch_load(const T* q, T (&x)[N]) {
    __builtin_memcpy(x, __builtin_assume_aligned(q, 8), sizeof(T) * N);
}

// The N sums one thread owns: output row `o`, input rows base + member row; fl, W: the time group's flags and the
// cell's total weight.  SUM01: a member's sample is x[s][0] + x[s][1] (Coherence -> Intensity), formed in f64
template <typename T, bool SUM01, int N>
__device__ __forceinline__ void scrunch_sums(const ScrunchArgs& a, const T* base, size_t polstep, int m, int m1, int fl, double W, double* o) {
    constexpr int U = SUM01 ? PP_SCRUNCH_UNROLL / 2 : PP_SCRUNCH_UNROLL;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    if (fl & 1) __builtin_memcpy(acc, __builtin_assume_aligned(o, 16), 8 * N);      // (f64 rows of even length start on 16 bytes)
    for (; m + U <= m1; m += U) {
        ScrunchMember mm[U];
        T x[U][N], y[SUM01 ? U : 1][N];
#pragma unroll
        for (int u = 0; u < U; ++u) mm[u] = a.mem[m + u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T* r = base + (size_t)mm[u].row * a.nbin;
            scrunch_load<T, N>(r, x[u]);
            if (SUM01) scrunch_load<T, N>(r + polstep, y[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < N; ++j)
                acc[j] = fma(mm[u].w, SUM01 ? (double)x[u][j] + (double)y[u][j] : (double)x[u][j], acc[j]);
    }
    for (; m < m1; ++m) {
        const ScrunchMember mm = a.mem[m];
        T x[N], y[N];
        const T* r = base + (size_t)mm.row * a.nbin;
        scrunch_load<T, N>(r, x);
        if (SUM01) scrunch_load<T, N>(r + polstep, y);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = fma(mm.w, SUM01 ? (double)x[j] + (double)y[j] : (double)x[j], acc[j]);
    }
    if (fl & 2) {
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = W > 0.0 ? acc[j] / W : 0.0;
    }
    __builtin_memcpy(__builtin_assume_aligned(o, 16), acc, 8 * N);
}

template <typename T, bool SUM01>
__global__ __launch_bounds__(256) void k_scrunch(ScrunchArgs a) {
    constexpr int V = 16 / (int)sizeof(T);
    const int nv = (a.nbin + V - 1) / V;
    const long long nitems = (long long)a.ngt * a.npo * a.ngf * nv;
    const size_t polstep = (size_t)a.nchan * a.nbin;
    const T* src = reinterpret_cast<const T*>(a.src);
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < nitems; item += (long long)gridDim.x * blockDim.x) {
        const long long orow = item / nv;
        const int b0 = (int)(item - orow * nv) * V;
        const int gf = (int)(orow % a.ngf);
        const long long gp = orow / a.ngf;
        const int p = (int)(gp % a.npo), gt = (int)(gp / a.npo);
        const int cell = gt * a.ngf + gf;
        const int fl = a.tflag[gt], m = a.off[cell], m1 = a.off[cell + 1];
        const double W = a.wtot[cell];
        double* o = a.out + (size_t)orow * a.nbin + b0;
        const T* base = src + (size_t)p * polstep + b0;
        // (nbin is even: the tail of an f32 row holds two samples, an f64 row has none)
        if (V == 2 || b0 + V <= a.nbin) scrunch_sums<T, SUM01, V>(a, base, polstep, m, m1, fl, W, o);
        else scrunch_sums<T, SUM01, 2>(a, base, polstep, m, m1, fl, W, o);
    }
}

}  // namespace pp
