// prach_noma_census.hip — the two kernels over THE NOMA MENU of include/prach.h, reduced on the device from the 64-byte per-UE log records prach::noma_kernel
// writes there, the trial's arrival schedule and its `steps`.  gfx950 only.
//   prach::noma_census_kernel   per trial group a two-axis cross-tabulation with a choice of classes (prach_run_trials_noma_census);
//                               prach_noma_census_accumulate_logs (prach_host.c) is the definition
//   prach::noma_columns_kernel  per UE of every trial the asked-for fields and raw record words as int32 columns (prach_run_trials_noma_columns, _device);
//                               prach_noma_columns_from_logs is the definition
// Both equal their definition integer for integer.  They have the shape of prach::xtab_kernel and prach::columns_kernel and share everything those share
// (prach_reduce_tile.h: tile, jobs, slot range, folds, flush); the menu is prach_noma_menu.h.  They are bodies of their own, not instantiations of one
// template with the two existing kernels: NOMA has four classes where the menu of prach_xtab_menu.h has three (one scalar more per group and per trial) and
// takes its class from other record quarters, so a shared body would be parameterised on the loads, the class, the scalar row and the value — all of it —
// and the existing kernels' code objects would no longer be the ones the project has measured and pinned.
//
// A workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial; TimelineJob::pad carries E = min(steps, maxTime).  A lane always reads words 8-11
// (preambleChange = the sector, maxRarCounter, preambleTxCounter) and 12-15 (connectionRequest, msg4Flag, failCount) of a record: the class needs them.
// Words 0-3 and 4-7 only where a field needs them (nm_needs_q0, nm_needs_q1): uniform for the launch, so a launch moves 32-64 B per UE.
//
// CENSUS, two paths by the size of the table, as in prach_xtab.hip: at most XT_WINDOW_WORDS cells under scheme 1 — the whole table privatised in LDS as
// 32-bit cells (a tile adds at most TL_TILE to one), one copy per wavefront while the copies fit NC_COPY_WORDS words (STATE, SECTOR or ONE on an axis puts a
// wavefront on one to nine addresses), non-zero cells flushed with 64-bit agent-scope atomic adds; a larger table, and everything under scheme 0, straight
// to its global cell with the same atomics.  The scalars are folded per wavefront.  Engine option "xtab_scheme".
// COLUMNS: one 4-byte store per lane and column, consecutive lanes at consecutive addresses; a trial's offset is any number of rows, so nothing is wider
// than a word.  Plain stores: a trial has a job only in the launch whose result is kept.
#include "prach_reduce_tile.h"
#include "prach_noma_menu.h"

namespace prach {

namespace {

constexpr int NC_COPY_WORDS = 4096; // LDS words that the per-wavefront copies of a table take at most (prach_xtab.hip's measured limit)
constexpr int NC_WAVES = TL_THREADS / 64;
static_assert(4 * (TILE_SCHED_CAP + 2 * NC_SCALARS + XT_WINDOW_WORDS) <= 160 * 1024 && NC_COPY_WORDS <= XT_WINDOW_WORDS,
              "the largest layout (a table of XT_WINDOW_WORDS cells) fits the 160 KiB of LDS of a gfx950 CU");

template <int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void noma_census_kernel(const TimelineJob *__restrict__ jobs, int njobs, XtabAxes ax, int copies, XtabOut out) {
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | NC_SCALARS x 64-bit scalars | path 1: [copies][ncell] cells
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const lcell = lds + TILE_SCHED_CAP + 2 * NC_SCALARS;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    const unsigned W = (unsigned)ax.col_bins + 1u, ncell = ((unsigned)ax.row_bins + 1u) * W; // (the engine refuses a table of more than 2^27 cells)
    const bool priv = SCHEME == 1 && ncell <= (unsigned)XT_WINDOW_WORDS;                      // path 1
    const bool need_a = nm_needs_arrival(ax.row_field) || nm_needs_arrival(ax.col_field);
    const bool need_q0 = nm_needs_q0(ax.row_field) || nm_needs_q0(ax.col_field);
    const bool need_q1 = nm_needs_q1(ax.row_field) || nm_needs_q1(ax.col_field);

    // the tile's slot range, only where an axis needs it: no search and no copy otherwise
    TileSlots S{0, 0, J.sched, 0};
    if (need_a) S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (priv)
        for (unsigned w = tid; w < ncell * (unsigned)copies; w += TL_THREADS) lcell[w] = 0;
    if (tid < NC_SCALARS) lsc[tid] = 0;
    __syncthreads();

    unsigned long long *const g_cell = out.cells + (size_t)J.group * (size_t)ncell;
    unsigned *const mycell = lcell + (copies > 1 ? (unsigned)(tid >> 6) * ncell : 0u);
    unsigned nidle = 0, nserved = 0, ndropped = 0, npending = 0, nsel = 0, nbinned = 0;
    unsigned long long rsum = 0, csum = 0, rmax1 = 0, cmax1 = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        int4 q0 = make_int4(0, 0, 0, 0), q1 = make_int4(0, 0, 0, 0);
        if (need_q0) q0 = J.logs[4 * (size_t)i];     // idx, timer, active, txTime
        if (need_q1) q1 = J.logs[4 * (size_t)i + 1]; // firstTxTime, secondTxTime, nowBackoff, preamble
        const int4 q2 = J.logs[4 * (size_t)i + 2];   // preambleChange (sector), rarWindow, maxRarCounter, preambleTxCounter
        const int4 q3 = J.logs[4 * (size_t)i + 3];   // msg2Flag, connectionRequest, msg4Flag, failCount
        const int cls = nm_class(q2, q3);
        nidle += cls == PRACH_NOMA_IDLE; nserved += cls == PRACH_NOMA_SERVED; ndropped += cls == PRACH_NOMA_DROPPED; npending += cls == PRACH_NOMA_PENDING;
        if (!(ax.who & cls)) continue;
        nsel++;
        const int a = need_a ? S.arrival(J, i) : 0;
        const long long rv = nm_value(ax.row_field, q0, q1, q2, q3, cls, a, E), cv = nm_value(ax.col_field, q0, q1, q2, q3, cls, a, E);
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
    nidle = fold_sum(nidle); nserved = fold_sum(nserved); ndropped = fold_sum(ndropped); npending = fold_sum(npending); nsel = fold_sum(nsel); nbinned = fold_sum(nbinned);
    rsum = fold_sum(rsum); csum = fold_sum(csum); rmax1 = fold_max(rmax1); cmax1 = fold_max(cmax1);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)nidle); atomicAdd(&lsc[1], (unsigned long long)nserved); atomicAdd(&lsc[2], (unsigned long long)ndropped);
        atomicAdd(&lsc[3], (unsigned long long)npending); atomicAdd(&lsc[4], (unsigned long long)nsel); atomicAdd(&lsc[5], (unsigned long long)nbinned);
        atomicAdd(&lsc[6], rsum); atomicAdd(&lsc[7], csum);
        atomicMax(&lsc[8], rmax1); atomicMax(&lsc[9], cmax1);
    }
    __syncthreads();

    // flush: only what this tile touched
    if (priv)
        for (unsigned w = tid; w < ncell; w += TL_THREADS) {
            unsigned v = lcell[w];
            for (int k = 1; k < copies; k++) v += lcell[(unsigned)k * ncell + w];
            if (v) agent_add(&g_cell[w], (unsigned long long)v);
        }
    flush_scalars(lsc, out.scalars + (size_t)J.group * NC_SCALARS, NC_SUMS, NC_MAXIMA, tid);
}

// word w (0 .. 15) of a record from its four quarters; w is uniform
__device__ __forceinline__ int record_word(int w, const int4 &q0, const int4 &q1, const int4 &q2, const int4 &q3) {
    const int4 q = (w >> 2) == 0 ? q0 : (w >> 2) == 1 ? q1 : (w >> 2) == 2 ? q2 : q3;
    return (w & 3) == 0 ? q.x : (w & 3) == 1 ? q.y : (w & 3) == 2 ? q.z : q.w;
}

__global__ __launch_bounds__(TL_THREADS) void noma_columns_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_columns_spec sp, ColumnsOut out) {
    __shared__ int lsched[TILE_SCHED_CAP];
    __shared__ unsigned long long lsc[NCL_SCALARS];
    const int tid = threadIdx.x, lane = tid & 63;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    // what the columns need, as 0 / 1
    int need_a = 0, need_q0 = 0, need_q1 = 0;
    for (int c = 0; c < sp.ncols; c++) {
        const int f = sp.field[c], w = f - PRACH_COL_RAW;
        need_a |= (int)nm_needs_arrival(f);
        need_q0 |= (int)nm_needs_q0(f) | (int)((w >> 2) == 0);
        need_q1 |= (int)nm_needs_q1(f) | (int)((w >> 2) == 1);
    }

    // the tile's slot range, only where a column needs it: no search and no copy otherwise
    TileSlots S{0, 0, J.sched, 0};
    if (need_a) S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (tid < NCL_SCALARS) lsc[tid] = 0;
    __syncthreads();

    int *const col0 = out.data + out.offset[J.group]; // the trial's segment of column 0
    unsigned nidle = 0, nserved = 0, ndropped = 0, npending = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        int4 q0 = make_int4(0, 0, 0, 0), q1 = make_int4(0, 0, 0, 0);
        if (need_q0) q0 = J.logs[4 * (size_t)i];
        if (need_q1) q1 = J.logs[4 * (size_t)i + 1];
        const int4 q2 = J.logs[4 * (size_t)i + 2];
        const int4 q3 = J.logs[4 * (size_t)i + 3];
        const int cls = nm_class(q2, q3);
        nidle += cls == PRACH_NOMA_IDLE; nserved += cls == PRACH_NOMA_SERVED; ndropped += cls == PRACH_NOMA_DROPPED; npending += cls == PRACH_NOMA_PENDING;
        const int a = need_a ? S.arrival(J, i) : 0;
        for (int c = 0; c < sp.ncols; c++) {
            const int f = sp.field[c];
            int v;
            if (f >= PRACH_COL_RAW) v = record_word(f - PRACH_COL_RAW, q0, q1, q2, q3);
            else {
                const long long x = nm_value(f, q0, q1, q2, q3, cls, a, E);
                v = x < 0 ? -1 : (int)x;
            }
            col0[(size_t)c * out.stride + (size_t)i] = v; // (i < nUE of the trial: inside its segment of the column)
        }
    }
    nidle = fold_sum(nidle); nserved = fold_sum(nserved); ndropped = fold_sum(ndropped); npending = fold_sum(npending);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)nidle); atomicAdd(&lsc[1], (unsigned long long)nserved); atomicAdd(&lsc[2], (unsigned long long)ndropped);
        atomicAdd(&lsc[3], (unsigned long long)npending);
    }
    __syncthreads();
    flush_scalars(lsc, out.scalars + (size_t)J.group * NCL_SCALARS, NCL_SUMS, 0, tid);
}

} // namespace

hipError_t launch_noma_census_kernel(const TimelineJob *jobs, int njobs, int workgroups, XtabAxes ax, int scheme, XtabOut out, hipStream_t stream) {
    const size_t ncell = ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const bool priv = scheme == 1 && ncell <= (size_t)XT_WINDOW_WORDS;
    const int copies = priv && ncell * NC_WAVES <= (size_t)NC_COPY_WORDS ? NC_WAVES : 1;
    const size_t lds = 4 * ((size_t)TILE_SCHED_CAP + 2 * NC_SCALARS + (priv ? ncell * (size_t)copies : 0));
    if (scheme == 0) return launch_with_lds(noma_census_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, ax, copies, out);
    return launch_with_lds(noma_census_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, ax, copies, out);
}
int noma_census_copy_words() { return NC_COPY_WORDS; }

hipError_t launch_noma_columns_kernel(const TimelineJob *jobs, int njobs, int workgroups, const prach_columns_spec &spec, ColumnsOut out, hipStream_t stream) {
    if (!prach_internal_noma_columns_spec_ok(&spec) || !out.data || !out.offset || !out.scalars) return hipErrorInvalidValue;
    hipLaunchKernelGGL(noma_columns_kernel, dim3(workgroups), dim3(TL_THREADS), 0, stream, jobs, njobs, spec, out);
    return hipGetLastError();
}

} // namespace prach
