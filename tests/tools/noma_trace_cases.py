"""prach::noma_trace_kernel (csrc/prach_noma_trace.hip) on rows no trial writes: the cases, the numpy restatement of the kernel's definition in int64, and the
glue around tests/tools/gpu_noma_trace_harness.hip (case file, child process, result file).  tests/test_noma_trace_cases_cpu.py checks the cases and the
reference without a GPU, tests/test_gpu_noma_trace_synthetic.py holds the kernel against them.  tests/tools/NOMA_TRACE.md has the file formats.  No GPU use and
no package import here."""
import os

import numpy as np

import harness as H

HARNESS = "gpu_noma_trace_harness.hip"
MAGIC, KIND, PATTERN, GUARD = 0x52445543, 21, 0x7FFF7FFF, 64
GUARD_WORD = (PATTERN << 32) | PATTERN
CONSTANTS = dict(NT_TILE=768, NT_THREADS=256, NT_WINDOW=128, NT_SCALARS=12)
TILE, WINDOW, NSC = CONSTANTS["NT_TILE"], CONSTANTS["NT_WINDOW"], CONSTANTS["NT_SCALARS"]
HUGE = 0x7FFFFFFF
ZERO, BIG, SMALL = range(3)


class Job:
    """One trial's rows [nrows, 8] (row r: slot r // 6, sector r % 6; words 6 and 7 are not the kernel's to read), its accessTime and its group."""

    def __init__(self, rows, access_time, group):
        self.rows, self.access_time, self.group = np.ascontiguousarray(rows, dtype=np.int32), int(access_time), int(group)
        assert self.rows.ndim == 2 and self.rows.shape[1] == 8 and len(self.rows) >= 1


class Case:
    def __init__(self, name, bins, bin_ms, ngroups, jobs):
        self.name, self.bins, self.bin_ms, self.ngroups, self.jobs = name, int(bins), int(bin_ms), int(ngroups), jobs

    def __repr__(self):
        return self.name

    def reference(self):
        """(series int64 [6, ngroups, 6, bins], scalars int64 [ngroups, NT_SCALARS]): the plain loop over the rows, in numpy.  A row's words are unsigned."""
        series = np.zeros((6, self.ngroups, 6, self.bins), dtype=np.int64)
        sc = np.zeros((self.ngroups, NSC), dtype=np.int64)
        for j in self.jobs:
            v = j.rows[:, :6].astype(np.uint32).astype(np.int64)
            r = np.arange(len(v), dtype=np.int64)
            slot, sec = r // 6, r % 6
            g = j.group
            sc[g, 0] += (len(v) + 5) // 6
            sc[g, 1:7] += v.sum(axis=0)
            sc[g, 8] = max(sc[g, 8], int(np.minimum(v[:, 0], 0xFFFFFFFE).max()) + 1)
            b = slot * j.access_time // self.bin_ms
            inside = b < self.bins
            sc[g, 7] += v[~inside, 0].sum()
            for q in range(6):
                np.add.at(series[q, g], (sec[inside], b[inside]), v[inside, q])
        return series, sc


def make_rows(rng, nrows, fill):
    """ZERO: nothing; BIG: every word of the record 2^31 - 1 - (r + q) % 3; SMALL: counts as a trial could leave them, two rows in three, zeros between.  Words 6
    and 7 hold a pattern in every fill: the kernel does not read them."""
    rows = np.zeros((nrows, 8), dtype=np.int64)
    r = np.arange(nrows)
    if fill == BIG:
        rows[:, :6] = HUGE - (r[:, None] + np.arange(6)[None, :]) % 3
    elif fill == SMALL:
        on = rng.integers(0, 3, nrows) > 0
        used = rng.integers(1, 55, nrows)
        singles = (rng.random(nrows) * (used + 1)).astype(np.int64)
        tx = 2 * used - singles + rng.integers(0, 9, nrows)
        granted = (rng.random(nrows) * (singles + 1)).astype(np.int64)
        pairs = granted // 2
        one = (rng.random(nrows) * (pairs + 1)).astype(np.int64)
        rows[:, :6] = np.where(on[:, None], np.stack([tx, used, singles, granted, pairs, one], axis=1), 0)
    rows[:, 6:] = PATTERN
    return rows.astype(np.int32)


def cases():
    rng = np.random.default_rng(20)
    T = TILE
    mk = lambda n, fill, aT, g: Job(make_rows(rng, n, fill), aT, g)
    out = [
        # trials of tile - 1, tile and tile + 1 rows, and of 1, 5, 6 and 7: a tile that ends inside a slot, a last tile of one row
        Case("tile_edges", (3 * T) // 6 + 2, 5, 3, [mk(T - 1, SMALL, 5, 0), mk(T, SMALL, 5, 1), mk(T + 1, SMALL, 5, 2), mk(1, SMALL, 5, 0), mk(5, SMALL, 5, 1), mk(6, SMALL, 5, 2), mk(7, SMALL, 5, 0)]),
        # rows near 2^31 - 1: one slot per bin, and three tiles and a bit into FOUR bins — the sums pass 2^32 in the window and in the global bins
        Case("huge_one_slot_per_bin", T // 6, 5, 1, [mk(T, BIG, 5, 0)]),
        Case("huge_four_bins", 4, 5 * ((3 * T + 11) // 6 // 4 + 1), 2, [mk(3 * T + 5, BIG, 5, 1), mk(T + 5, BIG, 5, 1)]),
        # bin_ms below accessTime: a tile's bins run past the LDS window (128 slots span 640 bins at 1 ms, 320 at 2 ms), with and without room for all of them
        Case("bin_below_slot_window_exceeded", 5 * ((2 * T + 7) // 6 + 1), 1, 2, [mk(2 * T + 7, SMALL, 5, 0), mk(T, BIG, 5, 1)]),
        Case("bin_below_slot_and_overflow", 500, 2, 2, [mk(2 * T + 1, SMALL, 5, 0), mk(T - 1, SMALL, 5, 1)]),
        # bin_ms above accessTime and no multiple of it; two accessTimes in one launch
        Case("bin_7_slot_5_and_10", 300, 7, 3, [mk(2 * T + 3, SMALL, 5, 0), mk(T + 6, SMALL, 10, 2), mk(T, SMALL, 5, 0)]),
        Case("bin_25", 60, 25, 1, [mk(2 * T, SMALL, 5, 0)]),
        Case("bin_wider_than_a_trial", 2, 100000, 2, [mk(777, SMALL, 5, 0), mk(3 * T + 3, SMALL, 5, 1)]),
        # everything behind the last bin: slot 0 is empty and bin 0 is all there is
        Case("everything_behind_the_last_bin", 1, 1, 2, [Job(np.concatenate([make_rows(rng, 6, ZERO), make_rows(rng, T + 1, SMALL)]), 5, 0), Job(np.concatenate([make_rows(rng, 6, ZERO), make_rows(rng, 12, BIG)]), 5, 1)]),
        Case("all_zero", 100, 50, 2, [mk(2 * T + 9, ZERO, 5, 0), mk(5, ZERO, 5, 1)]),
        # an empty group between two used ones, many small jobs
        Case("empty_group_many_jobs", 40, 5, 3, [mk(int(n), SMALL, 5, 2 * (k % 2)) for k, n in enumerate(rng.integers(1, 200, 300))]),
    ]
    return out


CASE_NAMES = ("tile_edges", "huge_one_slot_per_bin", "huge_four_bins", "bin_below_slot_window_exceeded", "bin_below_slot_and_overflow", "bin_7_slot_5_and_10", "bin_25",
              "bin_wider_than_a_trial", "everything_behind_the_last_bin", "all_zero", "empty_group_many_jobs")


def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def harness_constants(exe):
    return H.constants(exe)


def write_case(case, path):
    head = np.array([MAGIC, KIND, len(case.jobs), 0, case.bins, case.bin_ms, case.ngroups, 0], dtype=np.int32)
    rows = np.zeros((len(case.jobs), 8), dtype=np.int32)
    rows[:, :4] = [[len(j.rows), j.group, 1, j.access_time] for j in case.jobs]
    H.write_job_case(path, head, rows, [a for j in case.jobs for a in (np.full(len(j.rows), PATTERN, dtype=np.int32), j.rows.reshape(-1))])


def workgroups(case):
    return sum(-(-len(j.rows) // TILE) for j in case.jobs)


def read_result(case, path, scheme):
    """(series, scalars) of a result file; the header and every guard word are checked here."""
    w = np.fromfile(path, dtype="<u8")
    ser = case.ngroups * 6 * case.bins
    assert len(w) == 4 + 6 * (ser + GUARD) + case.ngroups * NSC + GUARD, len(w)
    assert w[:4].tolist() == [MAGIC, KIND, scheme, workgroups(case)], w[:4].tolist()
    body = w[4:]
    series = np.zeros((6, case.ngroups, 6, case.bins), dtype=np.int64)
    for q in range(6):
        part = body[q * (ser + GUARD):(q + 1) * (ser + GUARD)]
        assert (part[ser:] == GUARD_WORD).all(), f"guard behind series {q}"
        series[q] = part[:ser].astype(np.int64).reshape(case.ngroups, 6, case.bins)
    tail = body[6 * (ser + GUARD):]
    assert (tail[case.ngroups * NSC:] == GUARD_WORD).all(), "guard behind the scalars"
    return series, tail[:case.ngroups * NSC].astype(np.int64).reshape(case.ngroups, NSC)


def run_harness(exe, case, case_path, scheme, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"result_{scheme}.bin")
    H.run(exe, [case_path, res, scheme], timeout)
    return read_result(case, res, scheme)


def same(a, b):
    """None, or what differs first between two (series, scalars)."""
    for q in range(6):
        if not np.array_equal(a[0][q], b[0][q]):
            at = np.argwhere(a[0][q] != b[0][q])[0].tolist()
            return f"series {q} at [group, sector, bin] {at}: {a[0][q][tuple(at)]} != {b[0][q][tuple(at)]} ({int((a[0][q] != b[0][q]).sum())} differ)"
    if not np.array_equal(a[1], b[1]):
        at = np.argwhere(a[1] != b[1])[0].tolist()
        return f"scalars at [group, word] {at}: {a[1][tuple(at)]} != {b[1][tuple(at)]}"
    return None
