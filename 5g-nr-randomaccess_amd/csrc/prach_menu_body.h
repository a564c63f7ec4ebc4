// prach_menu_body.h — the bodies of the reducer kernels that work over a MENU of per-UE quantities, ONE copy each, as templates over the menu's policy
// (XtabMenu of prach_xtab_menu.h, NomaMenu of prach_noma_menu.h):
//   census_body<Menu, SCHEME>   prach::xtab_kernel (prach_xtab.hip), prach::noma_census_kernel (prach_noma_census.hip)
//   columns_body<Menu>          prach::columns_kernel (prach_columns.hip), prach::noma_columns_kernel (prach_noma_census.hip)
// and the three steps of the two-level selection that prach::summary_kernel (prach_summary.hip) and prach::noma_summary_kernel (prach_noma_select.hip) share
// around their own pass 1, pass 2 and row: select_coarse, select_fine_slots, select_level.  The __global__ functions keep their names, template parameters
// and arguments in their own files (the symbols that profiles, harnesses and the ISA inventory know) and only call a body.  What each kernel does, its LDS
// layout and its paths are described in its own file.  A policy states: NCLASSES, Needs {a, x, y} with needs(field) / needs(field, field) / needs_raw(word), Rec with load<WHOLE>(), cls(),
// bit(), counted() and value().  The two pick kernels are NOT here: as one body they were measurably slower (prach_noma_select.hip).  gfx950 only.
#pragma once
#include "prach_device.h"
#include "prach_device_fn.h"
#include "prach_reduce_tile.h"

namespace prach {

// ---- the census: a two-axis table per trial group (shape, paths and LDS layout: prach_xtab.hip) -------------------------------------------------------
// a group's scalar row, XT_SCALARS words: NCLASSES class counts, selected, binned, row_sum, col_sum | row_max + 1, col_max + 1 | spare
template <class Menu> constexpr int CENSUS_SUMS = Menu::NCLASSES + 4;

template <class Menu, int SCHEME>
__device__ __forceinline__ void census_body(const TimelineJob *jobs, int njobs, const XtabAxes &ax, int copies, const XtabOut &out) {
    constexpr int NC = Menu::NCLASSES;
    static_assert(NC == 3 || NC == 4, "three class counters, and a fourth where the menu has one");
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | XT_SCALARS x 64-bit scalars | path 1: [copies][ncell] cells
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const lcell = lds + TILE_SCHED_CAP + 2 * XT_SCALARS;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    const unsigned W = (unsigned)ax.col_bins + 1u, ncell = ((unsigned)ax.row_bins + 1u) * W; // (the engine refuses a table of more than 2^27 cells)
    const bool priv = SCHEME == 1 && ncell <= (unsigned)XT_WINDOW_WORDS;                      // path 1
    const typename Menu::Needs need = Menu::needs(ax.row_field, ax.col_field);

    // the tile's slot range, only where an axis needs it: no search and no copy otherwise
    TileSlots S{0, 0, J.sched, 0};
    if (need.a) S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (priv)
        for (unsigned w = tid; w < ncell * (unsigned)copies; w += TL_THREADS) lcell[w] = 0;
    if (tid < XT_SCALARS) lsc[tid] = 0;
    __syncthreads();

    unsigned long long *const g_cell = out.cells + (size_t)J.group * (size_t)ncell;
    unsigned *const mycell = lcell + (copies > 1 ? (unsigned)(tid >> 6) * ncell : 0u);
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0, nsel = 0, nbinned = 0; // (the class counters are scalars of their own: an array becomes a vector, and another loop)
    unsigned long long rsum = 0, csum = 0, rmax1 = 0, cmax1 = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const typename Menu::Rec u = Menu::template load<false>(J.logs, i, need);
        const int cls = Menu::cls(u);
        c0 += Menu::counted(cls, 0); c1 += Menu::counted(cls, 1); c2 += Menu::counted(cls, 2);
        if (NC > 3) c3 += Menu::counted(cls, 3);
        if (!(ax.who & Menu::bit(cls))) continue;
        nsel++;
        const int a = need.a ? S.arrival(J, i) : 0;
        const long long rv = Menu::value(ax.row_field, u, cls, a, E), cv = Menu::value(ax.col_field, u, cls, a, E);
        if (rv < 0 || cv < 0) continue; // UNDEFINED
        // (a value is below 2^31 + 6: it fits 32 unsigned bits, and the quotient is cut at the overflow bin)
        const unsigned r = min((unsigned)rv / (unsigned)ax.row_width, (unsigned)ax.row_bins), c = min((unsigned)cv / (unsigned)ax.col_width, (unsigned)ax.col_bins);
        const unsigned cell = r * W + c; // (r <= row_bins, c <= col_bins: below ncell)
        nbinned++;
        rsum += (unsigned long long)rv; csum += (unsigned long long)cv;
        rmax1 = max(rmax1, (unsigned long long)rv + 1ull); cmax1 = max(cmax1, (unsigned long long)cv + 1ull);
        if (priv) atomicAdd(&mycell[cell], 1u);
        else agent_add(&g_cell[cell], 1ull);
    }
    c0 = fold_sum(c0); c1 = fold_sum(c1); c2 = fold_sum(c2);
    if (NC > 3) c3 = fold_sum(c3);
    nsel = fold_sum(nsel); nbinned = fold_sum(nbinned);
    rsum = fold_sum(rsum); csum = fold_sum(csum); rmax1 = fold_max(rmax1); cmax1 = fold_max(cmax1);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)c0); atomicAdd(&lsc[1], (unsigned long long)c1); atomicAdd(&lsc[2], (unsigned long long)c2);
        if (NC > 3) atomicAdd(&lsc[3], (unsigned long long)c3);
        atomicAdd(&lsc[NC], (unsigned long long)nsel); atomicAdd(&lsc[NC + 1], (unsigned long long)nbinned); atomicAdd(&lsc[NC + 2], rsum); atomicAdd(&lsc[NC + 3], csum);
        atomicMax(&lsc[NC + 4], rmax1); atomicMax(&lsc[NC + 5], cmax1);
    }
    __syncthreads();

    // flush: only what this tile touched
    if (priv)
        for (unsigned w = tid; w < ncell; w += TL_THREADS) {
            unsigned v = lcell[w];
            for (int k = 1; k < copies; k++) v += lcell[(unsigned)k * ncell + w];
            if (v) agent_add(&g_cell[w], (unsigned long long)v);
        }
    flush_scalars(lsc, out.scalars + (size_t)J.group * XT_SCALARS, CENSUS_SUMS<Menu>, XT_MAXIMA, tid);
}

// ---- the columns: menu fields and raw record words of every UE (layout, loads and stores: prach_columns.hip) ------------------------------------------
// a trial's scalar row, CL_SCALARS words: NCLASSES class counts | spare
// word w (0 .. 15) of a record from its four quarters; w is uniform
__device__ __forceinline__ int record_word(int w, const int4 &q0, const int4 &q1, const int4 &q2, const int4 &q3) {
    const int4 q = (w >> 2) == 0 ? q0 : (w >> 2) == 1 ? q1 : (w >> 2) == 2 ? q2 : q3;
    return (w & 3) == 0 ? q.x : (w & 3) == 1 ? q.y : (w & 3) == 2 ? q.z : q.w;
}

template <class Menu>
__device__ __forceinline__ void columns_body(const TimelineJob *jobs, int njobs, const prach_columns_spec &sp, const ColumnsOut &out) {
    constexpr int NC = Menu::NCLASSES;
    static_assert((NC == 3 || NC == 4) && NC <= CL_SCALARS, "three class counters, and a fourth where the menu has one; a trial's scalar row holds them");
    __shared__ int lsched[TILE_SCHED_CAP];
    __shared__ unsigned long long lsc[CL_SCALARS];
    const int tid = threadIdx.x, lane = tid & 63;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    // what the columns need, as 0 / 1
    int na = 0, nx = 0, ny = 0;
    for (int c = 0; c < sp.ncols; c++) {
        const int f = sp.field[c];
        const typename Menu::Needs m = Menu::needs(f), r = Menu::needs_raw(f - PRACH_COL_RAW);
        na |= (int)m.a;
        nx |= (int)m.x | (int)r.x;
        ny |= (int)m.y | (int)r.y;
    }
    const typename Menu::Needs need{na != 0, nx != 0, ny != 0};

    // the tile's slot range, only where a column needs it: no search and no copy otherwise
    TileSlots S{0, 0, J.sched, 0};
    if (need.a) S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (tid < CL_SCALARS) lsc[tid] = 0;
    __syncthreads();

    int *const col0 = out.data + out.offset[J.group]; // the trial's segment of column 0
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const typename Menu::Rec u = Menu::template load<true>(J.logs, i, need);
        const int cls = Menu::cls(u);
        c0 += Menu::counted(cls, 0); c1 += Menu::counted(cls, 1); c2 += Menu::counted(cls, 2);
        if (NC > 3) c3 += Menu::counted(cls, 3);
        const int a = need.a ? S.arrival(J, i) : 0;
        for (int c = 0; c < sp.ncols; c++) {
            const int f = sp.field[c];
            int v;
            if (f >= PRACH_COL_RAW) v = record_word(f - PRACH_COL_RAW, u.q0, u.q1, u.q2, u.q3);
            else {
                const long long x = Menu::value(f, u, cls, a, E);
                v = x < 0 ? -1 : (int)x;
            }
            col0[(size_t)c * out.stride + (size_t)i] = v; // (i < nUE of the trial: inside its segment of the column)
        }
    }
    c0 = fold_sum(c0); c1 = fold_sum(c1); c2 = fold_sum(c2);
    if (NC > 3) c3 = fold_sum(c3);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)c0); atomicAdd(&lsc[1], (unsigned long long)c1); atomicAdd(&lsc[2], (unsigned long long)c2);
        if (NC > 3) atomicAdd(&lsc[3], (unsigned long long)c3);
    }
    __syncthreads();
    flush_scalars(lsc, out.scalars + (size_t)J.group * CL_SCALARS, NC, 0, tid);
}

// ---- the two-level selection: values 0 .. SM_MAX_VALUE as coarse << 6 | fine ---------------------------------------------------------------------------
constexpr int SEL_COARSE = 1024, SEL_FINE = 64;
static_assert(SEL_COARSE * SEL_FINE == SM_MAX_VALUE + 1 && SEL_COARSE % 64 == 0, "coarse << 6 | fine covers 0 .. SM_MAX_VALUE; a wavefront scans a coarse histogram in one go");

// the summaries' scan for one (quantity, level) target: ALL 64 lanes of one wavefront call (a DPP scan inside).  hist: the quantity's coarse histogram, r >= 1
// the rank wanted.  Leaves the coarse bin holding the rank and the rank left inside it; nothing where range errors left the histogram short of the rank
__device__ __forceinline__ void select_coarse(const unsigned *hist, long long r, int lane, int *coarse, unsigned *rem) {
    const unsigned *const h = hist + lane * (SEL_COARSE / 64);
    int s = 0;
#pragma unroll
    for (int b = 0; b < SEL_COARSE / 64; b++) s += (int)h[b];
    const int incl = wave_scan_incl(s), excl = incl - s;
    if ((long long)excl < r && r <= (long long)incl) { // one lane at most
        unsigned left = (unsigned)(r - excl);
        int b = 0;
        while (left > h[b]) left -= h[b++]; // (ends inside the lane's bins: their sum s >= left)
        *coarse = lane * (SEL_COARSE / 64) + b;
        *rem = left;
    }
}
// the fine histogram of every found target: that of the first target of its quantity (PRACH_SUMMARY_MAX_Q levels each) with the same coarse bin
template <int TARGETS> __device__ __forceinline__ void select_fine_slots(const int *tcoarse, int *tslot, int tid) {
    if (tid < TARGETS && tcoarse[tid] >= 0) {
        const int t0 = tid - tid % PRACH_SUMMARY_MAX_Q;
        int slot = tid;
        for (int u = tid - 1; u >= t0; u--)
            if (tcoarse[u] == tcoarse[tid]) slot = u;
        tslot[tid] = slot;
    }
}
// the value of target t: its coarse bin and the fine bin reaching the rank left; -1: not found
__device__ __forceinline__ long long select_level(const unsigned *lfine, const int *tcoarse, const unsigned *trem, const int *tslot, int t) {
    if (tcoarse[t] < 0) return -1;
    const unsigned *const f = lfine + tslot[t] * SEL_FINE;
    unsigned left = trem[t];
    int b = 0;
    while (b < SEL_FINE - 1 && left > f[b]) left -= f[b++];
    return ((long long)tcoarse[t] << 6) | b;
}

} // namespace prach
