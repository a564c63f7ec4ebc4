"""5g-nr-randomaccess_amd — MI355X-native PRACH random-access Monte-Carlo engine (host-side binding).

Thin ctypes binding of ``libprach_hip.so`` (C ABI: ``include/prach.h``).  The simulation itself runs
in hand-written HIP kernels (``csrc/prach_kernels.hip``); this module only marshals parameter
structs.  There is NO CPU fallback: if the library is not built or no gfx950 device is present the
calls raise.

The directory name is not a Python identifier; load it with ``__graft_entry__.load_package()`` or
``importlib`` (tests/conftest.py does), under the module name ``nr_randomaccess_amd``.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRACH_LIB") or os.path.join(HERE, "libprach_hip.so")  # PRACH_LIB: diagnostic builds only
CLI_PATH = os.path.join(HERE, "prach_sim")

VARIANT_BETA_C, VARIANT_WITHNOMA_C, VARIANT_NOMA_C = 0, 1, 2
RNG_GLIBC, RNG_PHILOX = 0, 1
FLAG_SECTOR_GRANTS, FLAG_NOMA_NONSECTOR = 1, 2
OK = 0


class PrachCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("variant", "uniform", "nUE", "nPreamble", "backoff", "nGrantUL",
                                         "maxRarWindow", "maxMsg2TxCount", "accessTime", "rng_mode")] + [
        ("seed", C.c_uint64), ("stream_offset", C.c_uint64), ("max_steps", C.c_int32), ("flags", C.c_int32),
        ("cellRadius", C.c_float), ("hBS", C.c_float), ("hUT", C.c_float)]


class PrachResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "time_exit", "maxTime", "nSuccessUE", "failedUEs",
                                         "preambleTxCount", "failCounts", "collisionPreambles", "totalPreambleTxop",
                                         "activeCheck", "nAccessUE", "continueFaliedUEs", "finalSuccessUEs")] + [
        ("totalDelay", C.c_float), ("sumTimer", C.c_int64), ("draws", C.c_uint64), ("steps", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


UE_FIELDS = ("idx", "timer", "active", "txTime", "firstTxTime", "secondTxTime", "nowBackoff", "preamble",
             "preambleChange", "rarWindow", "maxRarCounter", "preambleTxCounter", "msg2Flag",
             "connectionRequest", "msg4Flag", "failCount")


class PrachUeLog(C.Structure):
    _fields_ = [(n, C.c_int32) for n in UE_FIELDS]


class PrachTiming(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("upload_ms", C.c_double), ("total_ms", C.c_double),
                ("launches", C.c_int32), ("workgroups", C.c_int32), ("updates", C.c_uint64),
                ("cluster_size", C.c_int32), ("resident_limit", C.c_int32), ("fallback_trials", C.c_int32), ("spin_timeouts", C.c_int32),
                ("rec_mode", C.c_int32), ("xcd_packed", C.c_int32), ("group_visits", C.c_uint64), ("event_ues", C.c_uint64),
                ("trial_kernel_reruns", C.c_int32), ("noma_host_ues", C.c_int32), ("noma_gain_host_ues", C.c_int32), ("noma_gain_pad", C.c_int32), ("noma_gain_ms", C.c_double),
                ("noma_timeline_ms", C.c_double), ("noma_trace_ms", C.c_double), ("noma_summary_ms", C.c_double), ("noma_pick_ms", C.c_double), ("noma_census_ms", C.c_double), ("noma_columns_ms", C.c_double), ("columns_ms", C.c_double), ("pick_ms", C.c_double), ("xtab_ms", C.c_double), ("trace_ms", C.c_double), ("summary_ms", C.c_double), ("dist_ms", C.c_double), ("timeline_ms", C.c_double),
                ("sojourn_ms", C.c_double)]


DIST_PTC_BINS, DIST_MAX_DELAY_BINS = 256, 16384
DIST_FIELDS = ("trials", "ues", "success", "delay_overflow", "delay_sum", "ptc_sum", "delay_max")


class PrachDistSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("delay_bins", "delay_bin_ms", "ngroups", "reserved")]


class PrachDist(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in DIST_FIELDS[:-1]] + [("delay_max", C.c_int64)]


_U64P = C.POINTER(C.c_uint64)


class _Reduction:
    """What the grouped kinds share; csrc/prach_grouped.h states the same on the C side.  A subclass DECLARES its kind and implements nothing of it:

    _KIND     the name in prach_run_trials_<kind>, prach_<kind>_merge, prach_<kind>_format_csv and prach_<kind>_accumulate_logs
    _PARAMS   the constructor's arguments behind ngroups, (name, converter[, default]) each: they become attributes, and same_as and merge compare them
    _SPEC     the C struct of the spec, and _SPEC_OF, a function of the instance that gives its field values
    _STRUCT   the C struct of one group; _FIELDS its scalar fields, of which the last _MAXIMA start at -1; they are int64 arrays of length ngroups in the dict
              ``scalars`` (_SCALAR_ATTRS: attributes of their own instead)
    _NAMES    the uint64 arrays in the order of the C ABI, and _SHAPE, a function of the instance that gives the shape of one group of each
    _EXPOSE   how they are held: "attrs" an attribute [ngroups, *shape] per name, "dict" ``series[name]``, "stack" ONE array ``series`` [len(_NAMES), ngroups, *shape]
              (_VIEWS: and series[q] under its name)
    _RUN      how the device call and accumulate_logs take the arrays, _HOST how merge and CSV do: "flat" pointers, or one "array" uint64_t *[n]
    _LOGS     what accumulate_logs takes between the spec and the log: None (the kind has no host-side definition), "", "cfg" or "cfg,steps"
    """
    _MAXIMA, _SCALAR_ATTRS, _VIEWS, _RUN, _HOST, _LOGS, _NOUN = 1, False, False, "flat", "flat", None, "reductions"

    def __init__(self, ngroups, *args, **kw):
        import numpy as np
        self.ngroups = int(ngroups)
        if len(args) > len(self._PARAMS):
            raise TypeError(f"{type(self).__name__} takes ngroups and {len(self._PARAMS)} more arguments")
        for i, (name, conv, *default) in enumerate(self._PARAMS):
            if i >= len(args) and name not in kw and not default:
                raise TypeError(f"{type(self).__name__}: argument {name!r} is missing")
            setattr(self, name, conv(args[i] if i < len(args) else kw.pop(name, *default)))
        if kw:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(kw)}")
        shapes = self._SHAPE()
        if self._EXPOSE == "stack":
            self.series = np.zeros((len(self._NAMES), self.ngroups) + shapes[0], dtype=np.uint64)
            arrays = list(self.series)
        else:
            arrays = [np.zeros((self.ngroups,) + sh, dtype=np.uint64) for sh in shapes]
        if self._EXPOSE == "dict":
            self.series = dict(zip(self._NAMES, arrays))
        if self._EXPOSE == "attrs" or self._VIEWS:
            for n, a in zip(self._NAMES, arrays):
                setattr(self, n, a)
        scalars = {f: np.zeros(self.ngroups, dtype=np.int64) for f in self._FIELDS}
        for f in self._FIELDS[-self._MAXIMA:]:
            scalars[f][:] = -1
        if self._SCALAR_ATTRS:
            for f, a in scalars.items():
                setattr(self, f, a)
        else:
            self.scalars = scalars

    def spec(self):
        return self._SPEC(*self._SPEC_OF())

    def _arrays(self):
        """The [ngroups, ...] uint64 arrays in the order of the C ABI."""
        return [getattr(self, n) for n in self._NAMES] if self._EXPOSE == "attrs" else [self.series[n] for n in self._NAMES] if self._EXPOSE == "dict" else list(self.series)

    def _scalar(self, f):
        """The int64 array of length ngroups of scalar field f."""
        return getattr(self, f) if self._SCALAR_ATTRS else self.scalars[f]

    def _group(self, g):
        return self._STRUCT(*[int(self._scalar(f)[g]) for f in self._FIELDS])

    def _store(self, g, d):
        for f in self._FIELDS:
            self._scalar(f)[g] = getattr(d, f)

    def _ptrs(self, form, g=None):
        """The arrays — of group g, or of all groups — as the C side takes them in that form."""
        p = [(a if g is None else a[g]).ctypes.data_as(_U64P) for a in self._arrays()]
        return ((_U64P * len(p))(*p),) if form == "array" else tuple(p)

    def _rows(self, g):
        return list(self._ptrs("flat", g))

    def _series(self, g=None):
        """The arrays — of group g, or of all groups — as the uint64_t *[n] the C side takes."""
        return self._ptrs("array", g)[0]

    def _cargs(self, g):
        """Group g's arrays as the library's merge and CSV functions take them."""
        return self._ptrs(self._HOST, g)

    def merge_group(self, g, other, og):
        """Adds group ``og`` of ``other`` to group ``g`` (the kind's prach_*_merge)."""
        sp, a, b = self.spec(), self._group(g), other._group(og)
        getattr(lib(), f"prach_{self._KIND}_merge")(C.byref(sp), C.byref(a), *self._cargs(g), C.byref(b), *other._cargs(og))
        self._store(g, a)

    def _shape_key(self):
        return tuple(getattr(self, p[0]) for p in self._PARAMS)

    def merge(self, other):
        """Adds every group of ``other`` (same parameters and ngroups) to the same group of this one.  Returns self."""
        if (self._shape_key(), self.ngroups) != (other._shape_key(), other.ngroups):
            raise ValueError(f"{self._NOUN} of different shapes do not merge")
        for g in range(self.ngroups):
            self.merge_group(g, other, g)
        return self

    def csv(self, labels=None) -> bytes:
        """The CSV text of every group (the kind's prach_*_format_csv: asked for its size first, then filled), labelled labels[g] (default: the group number)."""
        out = b""
        sp, fmt = self.spec(), getattr(lib(), f"prach_{self._KIND}_format_csv")
        for g in range(self.ngroups):
            d = self._group(g)
            args = (C.byref(sp), C.byref(d), *self._cargs(g), str(g if labels is None else labels[g]).encode())
            need = fmt(*args, None, 0)
            buf = C.create_string_buffer(need + 1)
            n = fmt(*args, buf, need + 1)
            out += buf.raw[:n]
        return out

    def same_as(self, other):
        import numpy as np
        return self._shape_key() == other._shape_key() and all(np.array_equal(x, y) for x, y in zip(self._arrays(), other._arrays())) and \
            all(np.array_equal(self._scalar(f), other._scalar(f)) for f in self._FIELDS)

    @classmethod
    def from_logs(cls, logs, *params, cfgs=None, steps=None, groups=None, ngroups=None):
        """The kind's host-side definition (prach_*_accumulate_logs) over the logs: see _from_logs."""
        return _from_logs(cls(_ngroups(len(logs), groups, ngroups), *params), logs, groups, cfgs, steps)


class Dist(_Reduction):
    """The distributions of ``ngroups`` trial groups (include/prach.h, prach_dist): ``delay_hist`` [ngroups, delay_bins] and ``ptc_hist``
    [ngroups, 256] as numpy uint64, and one int64 array of length ngroups per scalar field of DIST_FIELDS."""
    _KIND, _PARAMS, _LOGS = "dist", (("delay_bins", int), ("delay_bin_ms", int, 1)), ""
    _SPEC, _SPEC_OF = PrachDistSpec, lambda s: (s.delay_bins, s.delay_bin_ms, s.ngroups, 0)
    _STRUCT, _FIELDS, _SCALAR_ATTRS = PrachDist, DIST_FIELDS, True
    _NAMES, _SHAPE, _EXPOSE = ("delay_hist", "ptc_hist"), lambda s: ((s.delay_bins,), (DIST_PTC_BINS,)), "attrs"

    def _hists(self, g):
        return tuple(self._rows(g))


TIMELINE_MAX_BINS = 65536
TIMELINE_SERIES = ("arrivals", "success", "sojourn_sum", "timer_sum", "done")
TIMELINE_FIELDS = ("trials", "ues", "arrived", "success", "restarted", "arrival_overflow", "done_overflow", "sojourn_sum", "timer_sum", "done_max")


class PrachTimelineSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bins", "bin_ms", "ngroups", "reserved")]


class PrachTimeline(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in TIMELINE_FIELDS[:-1]] + [("done_max", C.c_int64)]


class Timeline(_Reduction):
    """The timelines of ``ngroups`` trial groups (include/prach.h, prach_timeline): ``series[name]`` [ngroups, bins] as numpy uint64 for every name of
    TIMELINE_SERIES (bin b covers [b * bin_ms, (b + 1) * bin_ms)), and ``scalars[field]``, one int64 array of length ngroups per field of
    TIMELINE_FIELDS.  (Two dicts: `success` and `sojourn_sum` name a series and a scalar.)"""
    _KIND, _PARAMS, _HOST, _LOGS, _NOUN = "timeline", (("bins", int), ("bin_ms", int, 1)), "array", "cfg", "timelines"
    _SPEC, _SPEC_OF = PrachTimelineSpec, lambda s: (s.bins, s.bin_ms, s.ngroups, 0)
    _STRUCT, _FIELDS = PrachTimeline, TIMELINE_FIELDS
    _NAMES, _SHAPE, _EXPOSE = TIMELINE_SERIES, lambda s: ((s.bins,),) * 5, "dict"


SOJOURN_MAX_ARRIVAL_BINS, SOJOURN_MAX_DELAY_BINS = 4096, 16384
SOJOURN_FIELDS = ("trials", "ues", "arrived", "success", "restarted", "arrival_overflow", "delay_overflow", "sojourn_sum", "sojourn_max")


class PrachSojournSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("arrival_bins", "arrival_bin_ms", "delay_bins", "delay_bin_ms", "ngroups", "reserved")]


class PrachSojourn(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in SOJOURN_FIELDS[:-1]] + [("sojourn_max", C.c_int64)]


class Sojourn(_Reduction):
    """The sojourn histograms of ``ngroups`` trial groups (include/prach.h, prach_sojourn): ``hist`` [ngroups, arrival_bins, delay_bins], ``row_arrived`` and
    ``row_delay_overflow`` [ngroups, arrival_bins] as numpy uint64 (row r covers arrivals in [r * arrival_bin_ms, (r + 1) * arrival_bin_ms)), and
    ``scalars[field]``, one int64 array of length ngroups per field of SOJOURN_FIELDS."""
    _KIND, _LOGS = "sojourn", "cfg"
    _PARAMS = (("arrival_bins", int), ("arrival_bin_ms", int), ("delay_bins", int), ("delay_bin_ms", int, 1))
    _SPEC, _SPEC_OF = PrachSojournSpec, lambda s: (s.arrival_bins, s.arrival_bin_ms, s.delay_bins, s.delay_bin_ms, s.ngroups, 0)
    _STRUCT, _FIELDS = PrachSojourn, SOJOURN_FIELDS
    _NAMES, _SHAPE, _EXPOSE = ("hist", "row_arrived", "row_delay_overflow"), lambda s: ((s.arrival_bins, s.delay_bins), (s.arrival_bins,), (s.arrival_bins,)), "attrs"

    def quantile(self, g, row, q):
        """Lower edge (ms) of the delay bin holding the max(1, ceil(q * n))-th smallest sojourn of arrival row ``row`` of group g (row -1: pooled over all
        rows), n counting the row's overflow too; -1: no successful UE there, or that rank lies in the overflow (prach_sojourn_quantile)."""
        sp, (h, _, o) = self.spec(), self._rows(g)
        return int(lib().prach_sojourn_quantile(C.byref(sp), h, o, int(row), float(q)))


TRACE_MAX_BINS = 65536
TRACE_SERIES = ("calls", "singles", "txop", "collisions")
TRACE_FIELDS = ("trials", "subframes", "calls", "singles", "txop", "collisions", "overflow_calls", "calls_max")


class PrachTraceSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bins", "bin_ms", "ngroups", "reserved")]


class PrachTrace(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in TRACE_FIELDS[:-1]] + [("calls_max", C.c_int64)]


class Trace(_Reduction):
    """The per-subframe preamble traces of ``ngroups`` trial groups (include/prach.h, prach_trace): ``series[name]`` [ngroups, bins] as numpy uint64 for every
    name of TRACE_SERIES (bin b covers the subframes [b * bin_ms, (b + 1) * bin_ms)) — calls: preambles used, singles: preambles decoded, txop and
    collisions: what the subframes added to totalPreambleTxop and collisionPreambles, as the programs count them — and ``scalars[field]``, one int64
    array of length ngroups per field of TRACE_FIELDS.  There is no from_logs form: a per-UE log does not hold what happened per subframe."""
    _KIND, _PARAMS, _HOST, _NOUN = "trace", (("bins", int), ("bin_ms", int, 1)), "array", "traces"
    _SPEC, _SPEC_OF = PrachTraceSpec, lambda s: (s.bins, s.bin_ms, s.ngroups, 0)
    _STRUCT, _FIELDS = PrachTrace, TRACE_FIELDS
    _NAMES, _SHAPE, _EXPOSE = TRACE_SERIES, lambda s: ((s.bins,),) * 4, "dict"

    def collision_ratio(self, group):
        """(calls - singles) / calls per bin of one group, as float64: the share of the used preambles that collided (NaN where no preamble was used)."""
        import numpy as np
        c, s = self.series["calls"][group].astype(np.float64), self.series["singles"][group].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(c > 0, (c - s) / c, np.nan)


SUMMARY_MAX_Q = 8
SUMMARY_QUANTITIES = ("sojourn", "timer", "ptx")
SUMMARY_FIXED_METRICS = ("success_ratio", "restart_ratio", "sojourn_mean", "timer_mean", "ptx_mean")


class PrachSummarySpec(C.Structure):
    _fields_ = [("nq", C.c_int32), ("permille", C.c_int32 * SUMMARY_MAX_Q), ("reserved", C.c_int32 * 3)]


class PrachTrialSummary(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "nUE", "arrived", "success", "restarted", "range_errors")] + \
               [(n, C.c_int64) for n in ("sojourn_sum", "timer_sum", "ptc_sum")] + [(n, C.c_int32) for n in ("sojourn_max", "timer_max", "ptc_max")] + \
               [("q", (C.c_int32 * SUMMARY_MAX_Q) * 3)]


class PrachStat(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(n, C.c_double) for n in ("mean", "sd", "sem", "min", "max")]


def summary_row_dtype():
    """prach_trial_summary as a numpy structured dtype (the C layout: 160 bytes, twenty 64-bit words)."""
    import numpy as np
    dt = np.dtype([(n, np.int32) for n in ("status", "nUE", "arrived", "success", "restarted", "range_errors")] +
                  [(n, np.int64) for n in ("sojourn_sum", "timer_sum", "ptc_sum")] + [(n, np.int32) for n in ("sojourn_max", "timer_max", "ptc_max")] +
                  [("q", np.int32, (3, SUMMARY_MAX_Q))], align=True)
    assert dt.itemsize == C.sizeof(PrachTrialSummary)
    return dt


def summary_stat_dtype():
    import numpy as np
    return np.dtype([("n", np.uint64)] + [(n, np.float64) for n in ("mean", "sd", "sem", "min", "max")])


class Summary:
    """One row per trial (include/prach.h, prach_trial_summary): ``rows`` is a numpy structured array (summary_row_dtype) in trial order, ``permille`` the
    levels of its q[quantity][level] columns."""

    _FORMAT_CSV = "prach_summary_format_csv"

    def __init__(self, n, permille=(500, 950, 990)):
        import numpy as np
        self.permille = tuple(int(m) for m in permille)
        self.rows = np.zeros(int(n), dtype=summary_row_dtype())

    def spec(self):
        sp = PrachSummarySpec()
        sp.nq = len(self.permille)  # (a count the library refuses stays visible to it)
        for l, m in enumerate(self.permille[:SUMMARY_MAX_Q]):
            sp.permille[l] = m
        return sp

    def metric_names(self):
        return list(SUMMARY_FIXED_METRICS) + [f"{x}_p{m}" for x in SUMMARY_QUANTITIES for m in self.permille]

    def _rows_ptr(self):
        return self.rows.ctypes.data_as(C.POINTER(PrachTrialSummary))

    def _out_ptrs(self):
        return (self._rows_ptr(),)

    def stats(self, groups=None, ngroups=None):
        """Mean and spread per trial group (prach_summary_stats): a structured array [ngroups, 5 + 3 nq] of n, mean, sd, sem, min, max, the metrics in the
        order of metric_names().  groups: the group of every row (None: all rows are one group)."""
        import numpy as np
        ng = 1 if groups is None and ngroups is None else _ngroups(len(self.rows), groups, ngroups)
        out = np.zeros((ng, len(SUMMARY_FIXED_METRICS) + 3 * len(self.permille)), dtype=summary_stat_dtype())
        sp = self.spec()
        gp = None if groups is None else (C.c_int32 * len(self.rows))(*[int(g) for g in groups])
        rc = lib().prach_summary_stats(C.byref(sp), self._rows_ptr(), len(self.rows), gp, ng, out.ctypes.data_as(C.POINTER(PrachStat)))
        if rc != OK:
            raise PrachError(rc, "(prach_summary_stats)")
        return out


XTAB_SERVED, XTAB_UNSERVED, XTAB_IDLE = 1, 2, 4
XTAB_WHO = {"served": XTAB_SERVED, "unserved": XTAB_UNSERVED, "arrived": XTAB_SERVED | XTAB_UNSERVED, "idle": XTAB_IDLE, "all": XTAB_SERVED | XTAB_UNSERVED | XTAB_IDLE}
XTAB_FIELD_NAMES = ("one", "arrival", "sojourn", "completion", "timer", "ptc", "failcount", "age", "state")
XTAB_MAX_BINS = 65536
XTAB_FIELDS = ("trials", "ues", "idle", "served", "unserved", "selected", "binned", "undefined", "row_sum", "col_sum", "row_max", "col_max")


class PrachXtabSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("who", "row_field", "row_width", "row_bins", "col_field", "col_width", "col_bins", "ngroups")] + [("reserved", C.c_int32 * 2)]


class PrachXtab(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in XTAB_FIELDS[:-2]] + [("row_max", C.c_int64), ("col_max", C.c_int64)]


def xtab_axis(ax):
    """An axis of a cross-tabulation as (field id, width, bins): from such a tuple, whose field may be a name of XTAB_FIELD_NAMES, or from the text
    FIELD:WIDTH:BINS the drivers take."""
    f, w, b = ax.split(":") if isinstance(ax, str) else ax
    f = XTAB_FIELD_NAMES.index(f.lower()) if isinstance(f, str) and not f.lstrip("-").isdigit() else int(f)
    return f, int(w), int(b)


def xtab_parse_axis(text, max_time):
    """FIELD[:WIDTH[:BINS]] of the drivers as (field id, width, bins).  Defaults: width 500 for arrival, otherwise 1; as many bins as cover max_time (arrival)
    or max_time + 6 (the other times), 7 for state, 1 for one, 255 for ptc and failcount (prach_sim takes the same)."""
    parts = text.split(":")
    if not 1 <= len(parts) <= 3 or parts[0].lower() not in XTAB_FIELD_NAMES:
        raise ValueError(f"an axis is FIELD[:WIDTH[:BINS]], FIELD one of {', '.join(XTAB_FIELD_NAMES)}: {text!r}")
    f = XTAB_FIELD_NAMES.index(parts[0].lower())
    w = int(parts[1]) if len(parts) > 1 else 500 if f == 1 else 1
    if w < 1:
        raise ValueError(f"the width of an axis is at least 1: {text!r}")
    cover = {0: 1, 8: 7, 5: 255, 6: 255}.get(f, -(-(max_time + (0 if f == 1 else 6)) // w))
    b = int(parts[2]) if len(parts) > 2 else min(cover, XTAB_MAX_BINS)
    return f, w, b


class Xtab(_Reduction):
    """The outcome cross-tabulations of ``ngroups`` trial groups (include/prach.h, prach_xtab): ``cells`` [ngroups, row_bins + 1, col_bins + 1] as numpy uint64
    (the last index of an axis is its overflow bin) and ``scalars[field]``, one int64 array of length ngroups per field of XTAB_FIELDS.  rows, cols: an axis
    each, (field, width, bins); who: the classes that enter, bits XTAB_SERVED | XTAB_UNSERVED | XTAB_IDLE."""
    _KIND, _PARAMS, _LOGS = "xtab", (("rows", xtab_axis), ("cols", xtab_axis), ("who", int, XTAB_WHO["all"])), "cfg,steps"
    _SPEC, _SPEC_OF = PrachXtabSpec, lambda s: (s.who, *s.rows, *s.cols, s.ngroups, (C.c_int32 * 2)(0, 0))
    _STRUCT, _FIELDS, _MAXIMA = PrachXtab, XTAB_FIELDS, 2
    _NAMES, _SHAPE, _EXPOSE = ("cells",), lambda s: ((max(s.rows[2], 0) + 1, max(s.cols[2], 0) + 1),), "attrs"

    def cell_clauses(self, row_bin, col_bin):
        """The two clauses (field, lo, hi) of a pick (Engine.run_trials_pick, where=) that select exactly the UEs counted in cell [row_bin, col_bin]; the last
        bin of an axis is its overflow bin, which has no upper edge (hi is the largest int32)."""
        out = []
        for (f, w, b), bin_ in ((self.rows, int(row_bin)), (self.cols, int(col_bin))):
            if not 0 <= bin_ <= b:
                raise ValueError(f"bin {bin_} is not one of the {b} + 1 bins of the axis")
            out.append((f, bin_ * w, (bin_ + 1) * w - 1 if bin_ < b else 2 ** 31 - 1))
        return out

    def quantile(self, g, row, q):
        """Lower edge of the column bin holding the max(1, ceil(q * n))-th smallest column value of row ``row`` of group g (row -1: pooled over all rows), n
        counting the overflow column too; -1: nothing there, or that rank lies in the overflow column (prach_xtab_quantile)."""
        sp = self.spec()
        return int(lib().prach_xtab_quantile(C.byref(sp), self._rows(g)[0], int(row), float(q)))


PICK_MAX_K, PICK_MAX_CLAUSES = 4096, 4
PICK_ORDERS = {"index": 0, "largest": 1, "smallest": 2}
PICK_FIELDS = ("status", "nUE", "selected", "matched", "stored", "undefined", "range_errors", "threshold", "ties_left_out")


class PrachPickClause(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("field", "lo", "hi")]


class PrachPickSpec(C.Structure):
    _fields_ = [("who", C.c_int32), ("nclauses", C.c_int32), ("clause", PrachPickClause * PICK_MAX_CLAUSES)] + [(n, C.c_int32) for n in ("order", "key_field", "k", "reserved")]


class PrachPickRow(C.Structure):
    _fields_ = [("log", PrachUeLog), ("arrival", C.c_int32), ("key", C.c_int32), ("pad", C.c_int32 * 2)]


class PrachPick(C.Structure):
    _fields_ = [(n, C.c_int32) for n in PICK_FIELDS]


def pick_row_dtype():
    """prach_pick_row as a numpy structured dtype (80 bytes): the 16 logged fields by name, then arrival, key and two zero words."""
    import numpy as np
    dt = np.dtype([(n, np.int32) for n in UE_FIELDS + ("arrival", "key")] + [("pad", np.int32, (2,))])
    assert dt.itemsize == C.sizeof(PrachPickRow) == 80
    return dt


def pick_header_dtype():
    import numpy as np
    dt = np.dtype([(n, np.int32) for n in PICK_FIELDS])
    assert dt.itemsize == C.sizeof(PrachPick)
    return dt


def _xtab_field(f):
    return XTAB_FIELD_NAMES.index(f.lower()) if isinstance(f, str) and not f.lstrip("-").isdigit() else int(f)


def pick_parse_clause(text):
    """FIELD:LO:HI of the drivers as (field id, lo, hi)."""
    parts = text.split(":")
    if len(parts) != 3 or parts[0].lower() not in XTAB_FIELD_NAMES:
        raise ValueError(f"a clause is FIELD:LO:HI, FIELD one of {', '.join(XTAB_FIELD_NAMES)}: {text!r}")
    return XTAB_FIELD_NAMES.index(parts[0].lower()), int(parts[1]), int(parts[2])


class Pick:
    """The picks of ``n`` trials (include/prach.h, prach_pick): ``headers`` is a numpy structured array (pick_header_dtype) in trial order and ``rows`` one of
    shape [n, k] (pick_row_dtype); the first headers[t]["stored"] rows of trial t are its UEs in the defined order, the rows behind them are zero.
    where: up to four clauses (field, lo, hi), a field of XTAB_FIELD_NAMES; order: "index", "largest" or "smallest", the last two by the field ``key``;
    who: the classes that are selected, bits XTAB_SERVED | XTAB_UNSERVED | XTAB_IDLE."""

    def __init__(self, n, where=(), order="index", key=None, k=16, who=XTAB_WHO["all"]):
        import numpy as np
        self.where = tuple((self._field(f), int(lo), int(hi)) for f, lo, hi in where)
        self.order = PICK_ORDERS[order] if isinstance(order, str) else int(order)
        self.key = 0 if key is None else self._field(key)
        self.k, self.who = int(k), int(who)
        self.headers = np.zeros(int(n), dtype=pick_header_dtype())
        self.headers["threshold"] = -1
        self.rows = np.zeros((int(n), max(self.k, 1)), dtype=pick_row_dtype())

    _field = staticmethod(_xtab_field)  # a field name or id of this pick's menu

    def spec(self):
        sp = PrachPickSpec()
        sp.who, sp.nclauses, sp.order, sp.key_field, sp.k = self.who, len(self.where), self.order, self.key, self.k  # (a count the library refuses stays visible to it)
        for c, (f, lo, hi) in enumerate(self.where[:PICK_MAX_CLAUSES]):
            sp.clause[c] = PrachPickClause(f, lo, hi)
        return sp

    def _headers_ptr(self):
        return self.headers.ctypes.data_as(C.POINTER(PrachPick))

    def _rows_ptr(self, t=0):
        return C.cast(self.rows.ctypes.data + t * self.rows.strides[0], C.POINTER(PrachPickRow))

    def _out_ptrs(self):
        return self._headers_ptr(), self._rows_ptr()

    def same_as(self, other):
        import numpy as np
        return (self.where, self.order, self.key, self.k, self.who) == (other.where, other.order, other.key, other.k, other.who) and \
            all(np.array_equal(self.headers[f], other.headers[f]) for f in PICK_FIELDS) and all(np.array_equal(self.rows[f], other.rows[f]) for f in self.rows.dtype.names)


COL_MAX, COL_RAW, COL_MAX_WORDS = 16, 16, 1 << 31
COLUMNS_FIELDS = ("status", "nUE", "offset", "idle", "served", "unserved", "reserved")


class PrachColumnsSpec(C.Structure):
    _fields_ = [("ncols", C.c_int32), ("field", C.c_int32 * COL_MAX), ("reserved", C.c_int32 * 3)]


class PrachColumns(C.Structure):
    _fields_ = [("status", C.c_int32), ("nUE", C.c_int32), ("offset", C.c_uint64)] + [(n, C.c_int32) for n in ("idle", "served", "unserved", "reserved")]


def columns_header_dtype():
    import numpy as np
    dt = np.dtype([("status", np.int32), ("nUE", np.int32), ("offset", np.uint64)] + [(n, np.int32) for n in ("idle", "served", "unserved", "reserved")])
    assert dt.itemsize == C.sizeof(PrachColumns) == 32
    return dt


def columns_field(f):
    """A column's field id: a name of XTAB_FIELD_NAMES, ``raw:NAME`` with a field name of PrachUeLog (COL_RAW + its word), or the id itself."""
    if isinstance(f, str) and f.lower().startswith("raw:"):
        return COL_RAW + UE_FIELDS.index(f[4:])
    return _xtab_field(f)


def columns_field_name(f):
    return XTAB_FIELD_NAMES[f] if 0 <= f < len(XTAB_FIELD_NAMES) else "raw:" + UE_FIELDS[f - COL_RAW] if COL_RAW <= f < COL_RAW + 16 else str(f)


def columns_spec(fields):
    sp = PrachColumnsSpec()
    ids = [columns_field(f) for f in fields]
    sp.ncols = len(ids)  # (a count the library refuses stays visible to it)
    for c, f in enumerate(ids[:COL_MAX]):
        sp.field[c] = f
    return sp, ids


class Columns:
    """The per-UE columns of ``n`` trials (include/prach.h, prach_columns): ``data`` is [ncols, rows] int32 — a numpy array, or a torch CUDA tensor when the
    call was made with device=True — with trial k in the rows offsets[k] .. offsets[k] + nUE_k of every column; ``fields`` the columns' names (a name of
    XTAB_FIELD_NAMES or raw:NAME), ``headers`` a numpy structured array (columns_header_dtype) in trial order.  A menu field holds -1 where it is undefined,
    and every word of a trial that did not end PRACH_OK is -1."""

    def __init__(self, fields, headers, data):
        self.field_ids = tuple(columns_field(f) for f in fields)
        self.fields = tuple(columns_field_name(f) for f in self.field_ids)
        self.headers, self.data = headers, data
        self.offsets = headers["offset"].astype("int64")

    def trial(self, k):
        """[ncols, nUE_k]: the columns of trial k, a view."""
        o = int(self.offsets[k])
        return self.data[:, o:o + int(self.headers["nUE"][k])]

    def column(self, name):
        """[rows]: the (first) column of that field, a view."""
        return self.data[self.field_ids.index(columns_field(name))]


NOMA_SERVED, NOMA_PENDING, NOMA_IDLE, NOMA_DROPPED = 1, 2, 4, 8
NOMA_WHO = {"served": NOMA_SERVED, "pending": NOMA_PENDING, "dropped": NOMA_DROPPED, "idle": NOMA_IDLE, "arrived": NOMA_SERVED | NOMA_PENDING | NOMA_DROPPED,
            "all": NOMA_SERVED | NOMA_PENDING | NOMA_IDLE | NOMA_DROPPED}
NOMA_FIELD_NAMES = ("one", "arrival", "sojourn", "completion", "timer", "ptc", "retx", "msg3fail", "age", "state", "sector", "preamble", "lost")
NOMA_STATE_NAMES = ("idle", "served", "dropped", "backoff", "tx_ahead", "stranded", "msg3_pending", "msg3_timeout", "other")
NOMA_CENSUS_FIELDS = ("trials", "ues", "idle", "served", "dropped", "pending", "selected", "binned", "undefined", "row_sum", "col_sum", "row_max", "col_max")


class PrachNomaCensus(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in NOMA_CENSUS_FIELDS[:-2]] + [("row_max", C.c_int64), ("col_max", C.c_int64)]


class PrachNomaColumns(C.Structure):
    _fields_ = [("status", C.c_int32), ("nUE", C.c_int32), ("offset", C.c_uint64)] + [(n, C.c_int32) for n in ("idle", "served", "dropped", "pending")]


def noma_field(f):
    """A field id of the NOMA menu: a name of NOMA_FIELD_NAMES or the id itself."""
    return NOMA_FIELD_NAMES.index(f.lower()) if isinstance(f, str) and not f.lstrip("-").isdigit() else int(f)


def noma_axis(ax):
    """An axis of a NOMA census as (field id, width, bins): from such a tuple, whose field may be a name of NOMA_FIELD_NAMES, or from the text FIELD:WIDTH:BINS."""
    f, w, b = ax.split(":") if isinstance(ax, str) else ax
    return noma_field(f), int(w), int(b)


class NomaCensus(_Reduction):
    """The NOMA.c outcome census of ``ngroups`` trial groups (include/prach.h, prach_noma_census): ``cells`` [ngroups, row_bins + 1, col_bins + 1] as numpy uint64
    (the last index of an axis is its overflow bin) and ``scalars[field]``, one int64 array of length ngroups per field of NOMA_CENSUS_FIELDS.  rows, cols: an
    axis each, (field, width, bins), a field of NOMA_FIELD_NAMES; who: the classes that enter, bits NOMA_SERVED | NOMA_PENDING | NOMA_IDLE | NOMA_DROPPED."""
    _KIND, _PARAMS, _LOGS = "noma_census", (("rows", noma_axis), ("cols", noma_axis), ("who", int, NOMA_WHO["all"])), "cfg,steps"
    _SPEC, _SPEC_OF = PrachXtabSpec, Xtab._SPEC_OF
    _STRUCT, _FIELDS, _MAXIMA = PrachNomaCensus, NOMA_CENSUS_FIELDS, 2
    _NAMES, _SHAPE, _EXPOSE = ("cells",), Xtab._SHAPE, "attrs"

    def cell_clauses(self, row_bin, col_bin):
        """The two clauses (field, lo, hi) that describe exactly the UEs counted in cell [row_bin, col_bin] — NOMA field ids; the last bin of an axis is its
        overflow bin, which has no upper edge (hi is the largest int32).  They are the ``where`` of Engine.run_trials_noma_pick, whose ``matched`` is then the
        cell (with the census's ``who``), and they filter the columns of Engine.run_trials_noma_columns (lo <= column <= hi)."""
        out = []
        for (f, w, b), bin_ in ((self.rows, int(row_bin)), (self.cols, int(col_bin))):
            if not 0 <= bin_ <= b:
                raise ValueError(f"bin {bin_} is not one of the {b} + 1 bins of the axis")
            out.append((f, bin_ * w, (bin_ + 1) * w - 1 if bin_ < b else 2 ** 31 - 1))
        return out

    def quantile(self, g, row, q):
        """Xtab.quantile on this census's cells: prach_xtab_quantile reads only widths and bin counts, so it gets an xtab spec with those."""
        sp = PrachXtabSpec(XTAB_SERVED, 0, self.rows[1], self.rows[2], 0, self.cols[1], self.cols[2], self.ngroups, (C.c_int32 * 2)(0, 0))
        return int(lib().prach_xtab_quantile(C.byref(sp), self._rows(g)[0], int(row), float(q)))


NOMA_TRACE_SERIES = ("tx", "used", "singles", "granted", "pairs", "pair_one")
NOMA_TRACE_FIELDS = ("trials", "slots", "tx", "used", "singles", "granted", "pairs", "pair_one", "overflow_tx", "tx_max")


class PrachNomaTraceSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bins", "bin_ms", "ngroups", "reserved")]


class PrachNomaTrace(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in NOMA_TRACE_FIELDS[:-1]] + [("tx_max", C.c_int64)]


class NomaTrace(_Reduction):
    """NOMA.c's channel traces of ``ngroups`` trial groups (include/prach.h, prach_noma_trace): ``series`` [6, ngroups, 6 sectors, bins] as numpy uint64, in the
    order of NOMA_TRACE_SERIES (bin b covers the subframes [b * bin_ms, (b + 1) * bin_ms); an access slot counts where its subframe falls) — tx: preambles
    sent, used: (sector, preamble) bins with a transmitter, singles: bins with exactly one, granted: UEs whose msg2 was set, pairs: power-domain pairs that
    received a grant, pair_one: the pairs of which one UE decoded — and ``scalars[field]``, one int64 array of length ngroups per field of NOMA_TRACE_FIELDS.
    There is no from_logs form: a per-UE log does not hold what happened per slot."""
    _KIND, _PARAMS, _RUN, _HOST, _NOUN = "noma_trace", (("bins", int), ("bin_ms", int, 5)), "array", "array", "traces"
    _SPEC, _SPEC_OF = PrachNomaTraceSpec, lambda s: (s.bins, s.bin_ms, s.ngroups, 0)
    _STRUCT, _FIELDS = PrachNomaTrace, NOMA_TRACE_FIELDS
    _NAMES, _SHAPE, _EXPOSE = NOMA_TRACE_SERIES, lambda s: ((6, s.bins),) * 6, "stack"

    def named(self, name, group):
        """Series ``name`` of one group, summed over the sectors: [bins] float64."""
        import numpy as np
        return self.series[NOMA_TRACE_SERIES.index(name), group].sum(axis=0).astype(np.float64)

    def collision_ratio(self, group):
        """(used - singles) / used per bin of one group, all sectors, as float64: the share of the used (sector, preamble) bins that collided (NaN where none
        was used)."""
        import numpy as np
        u, s1 = self.named("used", group), self.named("singles", group)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(u > 0, (u - s1) / u, np.nan)

    def noma_share(self, group):
        """(2 * pairs - pair_one) / granted per bin of one group, all sectors, as float64: the share of the granted UEs that were granted through a power-domain
        pair (NaN where nobody was granted)."""
        import numpy as np
        g, p, o = self.named("granted", group), self.named("pairs", group), self.named("pair_one", group)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(g > 0, (2 * p - o) / g, np.nan)


NOMA_GAIN_MAX_BINS, NOMA_GAIN_NO_LEVEL = 4096, -2 ** 31
NOMA_GAIN_SERIES = ("arrived", "served", "dropped", "sojourn_sum", "lost_sum", "ptc_sum")
NOMA_GAIN_FIELDS = ("trials", "ues", "idle", "served", "dropped", "pending", "undefined", "below", "above", "restarted", "sojourn_sum", "lost_sum", "ptc_sum", "defined",
                    "level_max", "neg_level_max")


class PrachNomaGainSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bins", "width", "lo", "ngroups", "reserved")]


class PrachNomaGain(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in NOMA_GAIN_FIELDS[:-2]] + [("level_max", C.c_int64), ("neg_level_max", C.c_int64)]


class NomaGain(_Reduction):
    """NOMA.c's near-far profiles of ``ngroups`` trial groups (include/prach.h, prach_noma_gain): ``series`` [6, ngroups, 6 sectors, bins] as numpy uint64 in the
    order of NOMA_GAIN_SERIES — and each series under its name as a [ngroups, 6, bins] view — by the bin of the UE's GAIN LEVEL floor(1000 ln g): bin b covers the
    levels [lo + b * width, lo + (b + 1) * width); ``scalars[field]``, one int64 array of length ngroups per field of NOMA_GAIN_FIELDS (level_max and
    neg_level_max are -1 where ``defined`` is 0).  The sector is the UE's own, also under FLAG_NOMA_NONSECTOR."""
    _KIND, _PARAMS, _RUN, _HOST, _LOGS, _NOUN = "noma_gain", (("bins", int, 65), ("width", int, 200), ("lo", int, -16200)), "array", "array", "cfg,steps", "profiles"
    _SPEC, _SPEC_OF = PrachNomaGainSpec, lambda s: (s.bins, s.width, s.lo, s.ngroups, 0)
    _STRUCT, _FIELDS, _MAXIMA = PrachNomaGain, NOMA_GAIN_FIELDS, 2
    _NAMES, _SHAPE, _EXPOSE, _VIEWS = NOMA_GAIN_SERIES, lambda s: ((6, s.bins),) * 6, "stack", True

    def edges(self):
        """The lower edge of every bin, in level units (hundredths of 10 ln g): [bins] int64."""
        import numpy as np
        return self.lo + self.width * np.arange(self.bins, dtype=np.int64)

    def named(self, name, group, sector=None):
        """Series ``name`` of one group — of one sector, or summed over the sectors: [bins] float64."""
        import numpy as np
        a = self.series[NOMA_GAIN_SERIES.index(name), group]
        return (a.sum(axis=0) if sector is None else a[sector]).astype(np.float64)

    def _ratio(self, num, den):
        import numpy as np
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den > 0, num / den, np.nan)

    def served_ratio(self, g, sector=None):
        """served / arrived per gain bin of one group (one sector, or all), as float64; NaN where nobody arrived."""
        return self._ratio(self.named("served", g, sector), self.named("arrived", g, sector))

    def dropped_ratio(self, g, sector=None):
        """dropped / arrived per gain bin; NaN where nobody arrived."""
        return self._ratio(self.named("dropped", g, sector), self.named("arrived", g, sector))

    def mean_sojourn(self, g, sector=None):
        """sojourn_sum / served per gain bin, in ms: arrival to completion of the served UEs of that gain; NaN where none was served."""
        return self._ratio(self.named("sojourn_sum", g, sector), self.named("served", g, sector))

    def mean_lost(self, g, sector=None):
        """lost_sum / served per gain bin, in ms: arrival to the start of the last cycle; NaN where none was served."""
        return self._ratio(self.named("lost_sum", g, sector), self.named("served", g, sector))

    def mean_ptc(self, g, sector=None):
        """ptc_sum / served per gain bin: preamble transmissions of the served UEs of that gain; NaN where none was served."""
        return self._ratio(self.named("ptc_sum", g, sector), self.named("served", g, sector))


NOMA_TIMELINE_SERIES = ("arrivals", "served", "dropped", "sojourn_sum", "timer_sum", "done")
NOMA_TIMELINE_FIELDS = ("trials", "ues", "idle", "served", "dropped", "pending", "undefined", "restarted", "arrival_overflow", "done_overflow", "sojourn_sum", "timer_sum",
                        "done_max")


class PrachNomaTimelineSpec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bins", "bin_ms", "ngroups", "reserved")]


class PrachNomaTimeline(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in NOMA_TIMELINE_FIELDS[:-1]] + [("done_max", C.c_int64)]


class NomaTimeline(_Reduction):
    """NOMA.c's timelines per sector of ``ngroups`` trial groups (include/prach.h, prach_noma_timeline): ``series`` [6, ngroups, 6 sectors, bins] as numpy uint64
    in the order of NOMA_TIMELINE_SERIES, the layout of NomaTrace.series — and each series under its name as a [ngroups, 6, bins] view: ``arrivals``, ``served``,
    ``dropped``, ``sojourn_sum`` and ``timer_sum`` by the bin of the UE's ARRIVAL, ``done`` by the bin of its completion — and ``scalars[field]``, one int64 array
    of length ngroups per field of NOMA_TIMELINE_FIELDS.  The sector is the UE's own, also under FLAG_NOMA_NONSECTOR (where the trace has sector 0 only).
    A sojourn HISTOGRAM by arrival time is the census's: run_trials_noma_census with rows ARRIVAL, cols SOJOURN, who served, read with NomaCensus.quantile."""
    _KIND, _PARAMS, _RUN, _HOST, _LOGS, _NOUN = "noma_timeline", (("bins", int), ("bin_ms", int, 5)), "array", "array", "cfg,steps", "timelines"
    _SPEC, _SPEC_OF = PrachNomaTimelineSpec, lambda s: (s.bins, s.bin_ms, s.ngroups, 0)
    _STRUCT, _FIELDS = PrachNomaTimeline, NOMA_TIMELINE_FIELDS
    _NAMES, _SHAPE, _EXPOSE, _VIEWS = NOMA_TIMELINE_SERIES, lambda s: ((6, s.bins),) * 6, "stack", True

    def named(self, name, group, sector=None):
        """Series ``name`` of one group — of one sector, or summed over the sectors: [bins] float64."""
        import numpy as np
        a = self.series[NOMA_TIMELINE_SERIES.index(name), group]
        return (a.sum(axis=0) if sector is None else a[sector]).astype(np.float64)

    def _ratio(self, num, den):
        import numpy as np
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den > 0, num / den, np.nan)

    def served_ratio(self, g, sector=None):
        """served / arrivals per arrival bin of one group (one sector, or all), as float64; NaN where nobody arrived."""
        return self._ratio(self.named("served", g, sector), self.named("arrivals", g, sector))

    def dropped_ratio(self, g, sector=None):
        """dropped / arrivals per arrival bin; NaN where nobody arrived."""
        return self._ratio(self.named("dropped", g, sector), self.named("arrivals", g, sector))

    def mean_sojourn(self, g, sector=None):
        """sojourn_sum / served per arrival bin, in ms: arrival to completion of the served UEs that arrived there; NaN where none was served."""
        return self._ratio(self.named("sojourn_sum", g, sector), self.named("served", g, sector))

    def mean_lost(self, g, sector=None):
        """(sojourn_sum - timer_sum) / served per arrival bin, in ms: arrival to the start of the last attempt cycle; NaN where none was served."""
        return self._ratio(self.named("sojourn_sum", g, sector) - self.named("timer_sum", g, sector), self.named("served", g, sector))


NOMA_SUMMARY_MAX_FIELDS = 4
NOMA_SUMMARY_FIXED_METRICS = ("served_ratio", "dropped_ratio", "pending_ratio", "restart_ratio")


class PrachNomaSummarySpec(C.Structure):
    _fields_ = [("who", C.c_int32), ("nfields", C.c_int32), ("field", C.c_int32 * NOMA_SUMMARY_MAX_FIELDS), ("nq", C.c_int32), ("permille", C.c_int32 * SUMMARY_MAX_Q),
                ("reserved", C.c_int32 * 2)]


class PrachNomaTrialSummary(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "nUE", "idle", "served", "dropped", "pending", "selected", "restarted", "range_errors", "reserved")] + \
               [("n", C.c_int32 * NOMA_SUMMARY_MAX_FIELDS), ("sum", C.c_int64 * NOMA_SUMMARY_MAX_FIELDS), ("max", C.c_int32 * NOMA_SUMMARY_MAX_FIELDS),
                ("q", (C.c_int32 * SUMMARY_MAX_Q) * NOMA_SUMMARY_MAX_FIELDS)]


def noma_summary_row_dtype():
    """prach_noma_trial_summary as a numpy structured dtype (the C layout: 232 bytes)."""
    import numpy as np
    dt = np.dtype([(n, np.int32) for n in ("status", "nUE", "idle", "served", "dropped", "pending", "selected", "restarted", "range_errors", "reserved")] +
                  [("n", np.int32, (NOMA_SUMMARY_MAX_FIELDS,)), ("sum", np.int64, (NOMA_SUMMARY_MAX_FIELDS,)), ("max", np.int32, (NOMA_SUMMARY_MAX_FIELDS,)),
                   ("q", np.int32, (NOMA_SUMMARY_MAX_FIELDS, SUMMARY_MAX_Q))], align=True)
    assert dt.itemsize == C.sizeof(PrachNomaTrialSummary) == 232
    return dt


class NomaSummary:
    """One row per NOMA.c trial (include/prach.h, prach_noma_trial_summary): ``rows`` is a numpy structured array (noma_summary_row_dtype) in trial order;
    ``fields`` the up to four fields of NOMA_FIELD_NAMES behind n[x], sum[x], max[x] and q[x][level], ``permille`` the levels, ``who`` the classes whose UEs
    enter (bits NOMA_SERVED | NOMA_PENDING | NOMA_IDLE | NOMA_DROPPED)."""

    _FORMAT_CSV = "prach_noma_summary_format_csv"

    def __init__(self, n, fields=("sojourn", "timer", "ptc", "lost"), who=NOMA_WHO["served"], permille=(500, 950, 990)):
        import numpy as np
        self.field_ids = tuple(noma_field(f) for f in fields)
        self.who, self.permille = int(who), tuple(int(m) for m in permille)
        self.rows = np.zeros(int(n), dtype=noma_summary_row_dtype())

    def spec(self):
        sp = PrachNomaSummarySpec()
        sp.who, sp.nfields, sp.nq = self.who, len(self.field_ids), len(self.permille)  # (a count the library refuses stays visible to it)
        for x, f in enumerate(self.field_ids[:NOMA_SUMMARY_MAX_FIELDS]):
            sp.field[x] = f
        for l, m in enumerate(self.permille[:SUMMARY_MAX_Q]):
            sp.permille[l] = m
        return sp

    @property
    def metric_names(self):
        names = [NOMA_FIELD_NAMES[f] if 0 <= f < len(NOMA_FIELD_NAMES) else str(f) for f in self.field_ids]
        return list(NOMA_SUMMARY_FIXED_METRICS) + [n + suffix for n in names for suffix in ["_mean"] + [f"_p{m}" for m in self.permille]]

    def _rows_ptr(self):
        return self.rows.ctypes.data_as(C.POINTER(PrachNomaTrialSummary))

    _out_ptrs = Summary._out_ptrs

    def stats(self, groups=None, ngroups=None):
        """Mean and spread per trial group (prach_noma_summary_stats): a structured array [ngroups, 4 + nfields (1 + nq)] of n, mean, sd, sem, min, max, the
        metrics in the order of metric_names.  groups: the group of every row (None: all rows are one group)."""
        import numpy as np
        ng = 1 if groups is None and ngroups is None else _ngroups(len(self.rows), groups, ngroups)
        out = np.zeros((ng, len(self.metric_names)), dtype=summary_stat_dtype())
        sp = self.spec()
        gp = None if groups is None else (C.c_int32 * len(self.rows))(*[int(g) for g in groups])
        rc = lib().prach_noma_summary_stats(C.byref(sp), self._rows_ptr(), len(self.rows), gp, ng, out.ctypes.data_as(C.POINTER(PrachStat)))
        if rc != OK:
            raise PrachError(rc, "(prach_noma_summary_stats)")
        return out


def noma_pick_parse_clause(text):
    """FIELD:LO:HI of the drivers as (field id, lo, hi), FIELD of the NOMA menu."""
    parts = text.split(":")
    if len(parts) != 3 or parts[0].lower() not in NOMA_FIELD_NAMES:
        raise ValueError(f"a clause is FIELD:LO:HI, FIELD one of {', '.join(NOMA_FIELD_NAMES)}: {text!r}")
    return NOMA_FIELD_NAMES.index(parts[0].lower()), int(parts[1]), int(parts[2])


class NomaPick(Pick):
    """The picks of ``n`` NOMA.c trials (include/prach.h, prach_run_trials_noma_pick): Pick's headers and rows over the NOMA menu.  where: up to four clauses
    (field, lo, hi), a field of NOMA_FIELD_NAMES; order and key as in Pick, the key a field of NOMA_FIELD_NAMES; who: bits NOMA_SERVED | NOMA_PENDING |
    NOMA_IDLE | NOMA_DROPPED."""
    _field = staticmethod(noma_field)

    def __init__(self, n, where=(), order="index", key=None, k=16, who=NOMA_WHO["all"]):
        super().__init__(n, where, order, key, k, who)


def noma_columns_header_dtype():
    import numpy as np
    dt = np.dtype([("status", np.int32), ("nUE", np.int32), ("offset", np.uint64)] + [(n, np.int32) for n in ("idle", "served", "dropped", "pending")])
    assert dt.itemsize == C.sizeof(PrachNomaColumns) == 32
    return dt


def noma_columns_field(f):
    """A NOMA column's field id: a name of NOMA_FIELD_NAMES, ``raw:NAME`` with a field name of PrachUeLog (COL_RAW + its word), or the id itself."""
    if isinstance(f, str) and f.lower().startswith("raw:"):
        return COL_RAW + UE_FIELDS.index(f[4:])
    return noma_field(f)


def noma_columns_field_name(f):
    return NOMA_FIELD_NAMES[f] if 0 <= f < len(NOMA_FIELD_NAMES) else "raw:" + UE_FIELDS[f - COL_RAW] if COL_RAW <= f < COL_RAW + 16 else str(f)


def noma_columns_spec(fields):
    sp = PrachColumnsSpec()
    ids = [noma_columns_field(f) for f in fields]
    sp.ncols = len(ids)  # (a count the library refuses stays visible to it)
    for c, f in enumerate(ids[:COL_MAX]):
        sp.field[c] = f
    return sp, ids


class NomaColumns(Columns):
    """Columns over the NOMA menu (include/prach.h, prach_noma_columns): fields are names of NOMA_FIELD_NAMES or raw:NAME, headers have noma_columns_header_dtype."""

    def __init__(self, fields, headers, data):
        self.field_ids = tuple(noma_columns_field(f) for f in fields)
        self.fields = tuple(noma_columns_field_name(f) for f in self.field_ids)
        self.headers, self.data = headers, data
        self.offsets = headers["offset"].astype("int64")

    def column(self, name):
        """[rows]: the (first) column of that field, a view."""
        return self.data[self.field_ids.index(noma_columns_field(name))]


class PrachError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        try:
            msg = lib().prach_strerror(status).decode()
        except Exception:  # pragma: no cover
            msg = "?"
        super().__init__(f"libprach_hip status {status} ({msg}) {what}")


_lib = None
_lib_before_torch = None  # whether libprach_hip.so was loaded before torch was imported (lib())


def hip_runtimes():
    """The files named libamdhip64.so* that are mapped into this process: more than one means two HIP runtimes, and a device pointer of one means nothing to
    the other."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({os.path.realpath(ln.split()[-1]) for ln in f if "libamdhip64.so" in ln})
    except OSError:
        return []


def lib():
    """Load libprach_hip.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                                    f"(make -C 5g-nr-randomaccess_amd/csrc); there is no CPU fallback")
        global _lib_before_torch
        _lib_before_torch = "torch" not in sys.modules
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.prach_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.prach_engine_destroy.argtypes = [vp]
        L.prach_engine_destroy.restype = None
        L.prach_engine_set.argtypes = [vp, C.c_char_p, C.c_int64]
        L.prach_run_trials.argtypes = [vp, C.POINTER(PrachCfg), C.c_int, C.POINTER(PrachResult), C.POINTER(C.POINTER(PrachUeLog))]
        L.prach_last_timing.argtypes = [vp, C.POINTER(PrachTiming)]
        u64p = C.POINTER(C.c_uint64)
        # the three or four public functions of every grouped kind, from the class declarations (_Reduction)
        cfgp, uep = C.POINTER(PrachCfg), C.POINTER(PrachUeLog)
        for R in (Dist, Timeline, Sojourn, Trace, Xtab, NomaCensus, NomaTrace, NomaTimeline, NomaGain):
            sp, gp, ptrs = C.POINTER(R._SPEC), C.POINTER(R._STRUCT), {"flat": [u64p] * len(R._NAMES), "array": [C.POINTER(u64p)]}
            getattr(L, f"prach_run_trials_{R._KIND}").argtypes = [vp, cfgp, C.c_int, C.POINTER(PrachResult), C.POINTER(uep), sp, C.POINTER(C.c_int32), gp] + ptrs[R._RUN]
            merge, fmt = getattr(L, f"prach_{R._KIND}_merge"), getattr(L, f"prach_{R._KIND}_format_csv")
            merge.argtypes, merge.restype = [sp, gp] + ptrs[R._HOST] + [gp] + ptrs[R._HOST], None
            fmt.argtypes, fmt.restype = [sp, gp] + ptrs[R._HOST] + [C.c_char_p, C.c_char_p, C.c_size_t], C.c_size_t
            if R._LOGS is not None:
                getattr(L, f"prach_{R._KIND}_accumulate_logs").argtypes = [sp] + {"": [], "cfg": [cfgp], "cfg,steps": [cfgp, C.c_uint64]}[R._LOGS] + [uep, C.c_int, gp] + ptrs[R._RUN]
        L.prach_dist_delay_quantile.argtypes = [C.POINTER(PrachDistSpec), C.POINTER(PrachDist), u64p, C.c_double]
        L.prach_dist_delay_quantile.restype = C.c_int64
        L.prach_dist_tile_ues.argtypes = []
        L.prach_timeline_tile_ues.argtypes = []
        L.prach_timeline_window_bins.argtypes = []
        L.prach_sojourn_quantile.argtypes = [C.POINTER(PrachSojournSpec), u64p, u64p, C.c_int, C.c_double]
        L.prach_sojourn_quantile.restype = C.c_int64
        L.prach_sojourn_tile_ues.argtypes = []
        L.prach_sojourn_window_words.argtypes = []
        L.prach_xtab_quantile.argtypes = [C.POINTER(PrachXtabSpec), u64p, C.c_int, C.c_double]
        L.prach_xtab_quantile.restype = C.c_int64
        L.prach_xtab_tile_ues.argtypes = []
        L.prach_xtab_window_words.argtypes = []
        L.prach_run_trials_summary.argtypes = [vp, C.POINTER(PrachCfg), C.c_int, C.POINTER(PrachResult), C.POINTER(C.POINTER(PrachUeLog)), C.POINTER(PrachSummarySpec),
                                               C.POINTER(PrachTrialSummary)]
        L.prach_summary_from_logs.argtypes = [C.POINTER(PrachSummarySpec), C.POINTER(PrachCfg), C.POINTER(PrachUeLog), C.c_int, C.POINTER(PrachTrialSummary)]
        L.prach_summary_stats.argtypes = [C.POINTER(PrachSummarySpec), C.POINTER(PrachTrialSummary), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(PrachStat)]
        L.prach_summary_format_csv.argtypes = [C.POINTER(PrachSummarySpec), C.POINTER(PrachStat), C.c_char_p, C.c_char_p, C.c_size_t]
        L.prach_summary_format_csv.restype = C.c_size_t
        L.prach_summary_max_value.argtypes = []
        L.prach_run_trials_pick.argtypes = [vp, C.POINTER(PrachCfg), C.c_int, C.POINTER(PrachResult), C.POINTER(C.POINTER(PrachUeLog)), C.POINTER(PrachPickSpec),
                                            C.POINTER(PrachPick), C.POINTER(PrachPickRow)]
        L.prach_pick_from_logs.argtypes = [C.POINTER(PrachPickSpec), C.POINTER(PrachCfg), C.c_uint64, C.POINTER(PrachUeLog), C.c_int, C.POINTER(PrachPick), C.POINTER(PrachPickRow)]
        L.prach_pick_format_csv.argtypes = [C.POINTER(PrachPickSpec), C.POINTER(PrachPick), C.POINTER(PrachPickRow), C.c_char_p, C.c_int, C.c_uint64, C.c_char_p, C.c_size_t]
        L.prach_pick_format_csv.restype = C.c_size_t
        L.prach_run_trials_columns.argtypes = [vp, C.POINTER(PrachCfg), C.c_int, C.POINTER(PrachResult), C.POINTER(C.POINTER(PrachUeLog)), C.POINTER(PrachColumnsSpec),
                                               C.POINTER(PrachColumns), C.c_void_p, C.c_uint64]
        L.prach_run_trials_columns_device.argtypes = L.prach_run_trials_columns.argtypes
        L.prach_columns_from_logs.argtypes = [C.POINTER(PrachColumnsSpec), C.POINTER(PrachCfg), C.c_uint64, C.POINTER(PrachUeLog), C.c_int, C.c_void_p, C.c_uint64]
        L.prach_columns_tile_ues.argtypes = []
        L.prach_noma_census_tile_ues.argtypes = []
        L.prach_run_trials_noma_columns.argtypes = [vp, C.POINTER(PrachCfg), C.c_int, C.POINTER(PrachResult), C.POINTER(C.POINTER(PrachUeLog)), C.POINTER(PrachColumnsSpec),
                                                    C.POINTER(PrachNomaColumns), C.c_void_p, C.c_uint64]
        L.prach_run_trials_noma_columns_device.argtypes = L.prach_run_trials_noma_columns.argtypes
        L.prach_run_trials_noma_summary.argtypes = [vp, C.POINTER(PrachCfg), C.c_int, C.POINTER(PrachResult), C.POINTER(C.POINTER(PrachUeLog)), C.POINTER(PrachNomaSummarySpec),
                                                    C.POINTER(PrachNomaTrialSummary)]
        L.prach_noma_summary_from_logs.argtypes = [C.POINTER(PrachNomaSummarySpec), C.POINTER(PrachCfg), C.c_uint64, C.POINTER(PrachUeLog), C.c_int, C.POINTER(PrachNomaTrialSummary)]
        L.prach_noma_summary_stats.argtypes = [C.POINTER(PrachNomaSummarySpec), C.POINTER(PrachNomaTrialSummary), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(PrachStat)]
        L.prach_noma_summary_format_csv.argtypes = [C.POINTER(PrachNomaSummarySpec), C.POINTER(PrachStat), C.c_char_p, C.c_char_p, C.c_size_t]
        L.prach_noma_summary_format_csv.restype = C.c_size_t
        L.prach_run_trials_noma_pick.argtypes = L.prach_run_trials_pick.argtypes
        L.prach_noma_pick_from_logs.argtypes = L.prach_pick_from_logs.argtypes
        L.prach_noma_pick_format_csv.argtypes = L.prach_pick_format_csv.argtypes
        L.prach_noma_pick_format_csv.restype = C.c_size_t
        L.prach_noma_columns_from_logs.argtypes = [C.POINTER(PrachColumnsSpec), C.POINTER(PrachCfg), C.c_uint64, C.POINTER(PrachUeLog), C.c_int, C.c_void_p, C.c_uint64]
        L.prach_trace_tile_subframes.argtypes = []
        L.prach_cfg_defaults.argtypes = [C.POINTER(PrachCfg), C.c_int]
        L.prach_cfg_defaults.restype = None
        L.prach_cfg_validate.argtypes = [C.POINTER(PrachCfg)]
        L.prach_max_time.argtypes = [C.POINTER(PrachCfg)]
        L.prach_trial_cost.argtypes = [C.POINTER(PrachCfg)]
        L.prach_trial_cost.restype = C.c_double
        L.prach_arrival_schedule.argtypes = [C.POINTER(PrachCfg), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]
        L.prach_glibc_stream.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        L.prach_glibc_stream.restype = None
        L.prach_device_glibc_stream.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        L.prach_strerror.argtypes = [C.c_int]
        L.prach_strerror.restype = C.c_char_p
        L.prach_format_logs.argtypes = [C.POINTER(PrachUeLog), C.c_int, C.c_char_p, C.c_size_t]
        L.prach_format_logs.restype = C.c_size_t
        L.prach_format_results.argtypes = [C.POINTER(PrachCfg), C.POINTER(PrachResult), C.c_double, C.c_char_p, C.c_size_t]
        L.prach_format_results.restype = C.c_size_t
        L.prach_format_stdout.argtypes = [C.POINTER(PrachCfg), C.POINTER(PrachResult), C.c_double, C.c_char_p, C.c_size_t]
        L.prach_format_stdout.restype = C.c_size_t
        L.prach_result_file_name.argtypes = [C.POINTER(PrachCfg), C.c_int, C.c_char_p, C.c_size_t]
        L.prach_write_trial_files.argtypes = [C.POINTER(PrachCfg), C.POINTER(PrachResult), C.POINTER(PrachUeLog), C.c_double, C.c_char_p]
        L.prach_noma_activation_table.argtypes = [C.POINTER(PrachCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.prach_noma_activation_range.argtypes = [C.POINTER(PrachCfg), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.prach_noma_activation_table_device.argtypes = [C.c_void_p, C.POINTER(PrachCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.prach_format_noma_line.argtypes = [C.POINTER(PrachCfg), C.POINTER(PrachResult), C.c_char_p, C.c_size_t]
        L.prach_format_noma_line.restype = C.c_size_t
        L.prach_results_csv_accumulate.argtypes = [C.POINTER(C.c_double), C.c_char_p]
        L.prach_results_csv_row.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_char_p, C.c_size_t]
        L.prach_results_csv_row.restype = C.c_size_t
        L.prach_noma_trace_tile_rows.argtypes = []
        L.prach_noma_timeline_tile_ues.argtypes = []
        L.prach_noma_timeline_window_bins.argtypes = []
        L.prach_noma_gain_level.argtypes, L.prach_noma_gain_level.restype = [C.c_double], C.c_int32
        L.prach_noma_gain_levels.argtypes = [cfgp, C.c_void_p]
        L.prach_noma_gain_accumulate_levels.argtypes = [C.POINTER(PrachNomaGainSpec), cfgp, C.c_uint64, uep, C.c_int, C.c_void_p, C.POINTER(PrachNomaGain), C.POINTER(u64p)]
        L.prach_noma_gain_tile_ues.argtypes = []
        L.prach_noma_gain_lds_max_bins.argtypes = []
        _lib = L
    return _lib


EXPORTS = ("prach_engine_create", "prach_engine_destroy", "prach_engine_set", "prach_run_trials", "prach_last_timing",
           "prach_cfg_defaults", "prach_cfg_validate", "prach_max_time", "prach_trial_cost", "prach_arrival_schedule", "prach_glibc_stream",
           "prach_strerror", "prach_format_logs", "prach_format_results", "prach_format_stdout",
           "prach_result_file_name", "prach_write_trial_files", "prach_noma_activation_table", "prach_format_noma_line",
           "prach_results_csv_accumulate", "prach_results_csv_row", "prach_device_glibc_stream", "prach_noma_activation_range", "prach_noma_activation_stream",
           "prach_noma_activation_table_device", "prach_run_trials_dist", "prach_dist_accumulate_logs", "prach_dist_merge", "prach_dist_delay_quantile",
           "prach_dist_format_csv", "prach_dist_tile_ues", "prach_run_trials_timeline", "prach_timeline_accumulate_logs", "prach_timeline_merge",
           "prach_timeline_format_csv", "prach_timeline_tile_ues", "prach_timeline_window_bins", "prach_run_trials_sojourn", "prach_sojourn_accumulate_logs",
           "prach_sojourn_merge", "prach_sojourn_quantile", "prach_sojourn_format_csv", "prach_sojourn_tile_ues", "prach_sojourn_window_words",
           "prach_run_trials_summary", "prach_summary_from_logs", "prach_summary_stats", "prach_summary_format_csv", "prach_summary_max_value",
           "prach_run_trials_trace", "prach_trace_merge", "prach_trace_format_csv", "prach_trace_tile_subframes", "prach_run_trials_xtab", "prach_xtab_accumulate_logs",
           "prach_xtab_merge", "prach_xtab_quantile", "prach_xtab_format_csv", "prach_xtab_tile_ues", "prach_xtab_window_words", "prach_run_trials_pick",
           "prach_pick_from_logs", "prach_pick_format_csv", "prach_run_trials_columns", "prach_run_trials_columns_device", "prach_columns_from_logs",
           "prach_columns_tile_ues", "prach_run_trials_noma_census", "prach_noma_census_accumulate_logs", "prach_noma_census_merge", "prach_noma_census_format_csv",
           "prach_noma_census_tile_ues", "prach_run_trials_noma_columns", "prach_run_trials_noma_columns_device", "prach_noma_columns_from_logs",
           "prach_run_trials_noma_pick", "prach_noma_pick_from_logs", "prach_noma_pick_format_csv", "prach_run_trials_noma_summary", "prach_noma_summary_from_logs",
           "prach_noma_summary_stats", "prach_noma_summary_format_csv", "prach_run_trials_noma_trace", "prach_noma_trace_merge", "prach_noma_trace_format_csv",
           "prach_noma_trace_tile_rows", "prach_run_trials_noma_timeline", "prach_noma_timeline_accumulate_logs", "prach_noma_timeline_merge",
           "prach_noma_timeline_format_csv", "prach_noma_timeline_tile_ues", "prach_noma_timeline_window_bins", "prach_run_trials_noma_gain", "prach_noma_gain_level",
           "prach_noma_gain_levels", "prach_noma_gain_accumulate_levels", "prach_noma_gain_accumulate_logs", "prach_noma_gain_merge", "prach_noma_gain_format_csv",
           "prach_noma_gain_tile_ues", "prach_noma_gain_lds_max_bins")


def make_cfg(nUE, variant=VARIANT_BETA_C, uniform=0, rng_mode=RNG_GLIBC, seed=0, stream_offset=0, **kw) -> PrachCfg:
    """Defaults of the named program (Beta.c:47-57 / WithNOMA:70-88), overridden by keywords."""
    c = PrachCfg()
    lib().prach_cfg_defaults(C.byref(c), variant)
    c.nUE, c.uniform, c.rng_mode, c.seed, c.stream_offset = nUE, uniform, rng_mode, seed, stream_offset
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


class Engine:
    """One engine per process/GPU: owns the HIP stream and the device arena."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        self.device = int(device)
        rc = lib().prach_engine_create(device, C.byref(self._h))
        if rc != OK:
            raise PrachError(rc, "(prach_engine_create)")

    def close(self):
        if self._h:
            lib().prach_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, key: str, value: int):
        rc = lib().prach_engine_set(self._h, key.encode(), value)
        if rc != OK:
            raise PrachError(rc, f"(set {key})")

    def _call(self, name, cfgs, want_logs, *more):
        """What every prach_run_trials* call shares: the config array, the results, the log buffers, the status check.  Returns (results, logs)."""
        n = len(cfgs)
        arr = (PrachCfg * n)(*cfgs)
        res = (PrachResult * n)()
        logs, lp = self._log_buffers(cfgs, want_logs)
        rc = getattr(lib(), name)(self._h, arr, n, res, lp, *more)
        if rc != OK:
            raise PrachError(rc, f"({name})")
        return list(res), logs

    def _call_reduced(self, red, cfgs, groups, want_logs):
        """... with the grouped reduction `red` (a _Reduction), which takes what the device made.  Returns (results, logs, red)."""
        sp = red.spec()
        gg = (red._STRUCT * red.ngroups)()
        gp = None if groups is None else (C.c_int32 * len(cfgs))(*[int(g) for g in groups])
        res, logs = self._call(f"prach_run_trials_{red._KIND}", cfgs, want_logs, C.byref(sp), gp, gg, *red._ptrs(red._RUN))
        for g in range(red.ngroups):
            red._store(g, gg[g])
        return res, logs, red

    def _call_per_trial(self, name, out, cfgs, want_logs):
        """... with `out` (a Summary, a NomaSummary, a Pick or a NomaPick), whose rows per trial the device fills.  Returns (results, logs, out)."""
        sp = out.spec()
        res, logs = self._call(name, cfgs, want_logs, C.byref(sp), *out._out_ptrs())
        return res, logs, out

    def run_trials(self, cfgs, want_logs=False):
        """Run the trials concurrently on the device. Returns (results, logs) — logs[k] is a ctypes
        array of PrachUeLog or None.  want_logs: True (every trial), False, or the indices of the trials
        whose per-UE log is wanted (the C ABI takes NULL for the others)."""
        return self._call("prach_run_trials", cfgs, want_logs)

    def run_trials_dist(self, cfgs, delay_bins, delay_bin_ms=1, groups=None, want_logs=False, ngroups=None):
        """run_trials plus the distributions of access delay and preamble transmissions of the successful UEs, reduced on the device
        (prach_run_trials_dist).  groups: the group of every trial (None: one group per trial); ngroups: the number of groups (default: the
        largest group id + 1).  Returns (results, logs, Dist)."""
        return self._call_reduced(Dist(_ngroups(len(cfgs), groups, ngroups), delay_bins, delay_bin_ms), cfgs, groups, want_logs)

    def run_trials_timeline(self, cfgs, bins, bin_ms=1, groups=None, want_logs=False, ngroups=None):
        """run_trials plus the timelines per trial group — arrivals, successes, sojourn and timer sums by arrival time, completions by completion time —
        reduced on the device from the per-UE log records the simulation kernels leave there (prach_run_trials_timeline; Beta.c and
        RandomAccessWithNOMA trials only).  groups / ngroups / want_logs as in run_trials_dist.  Returns (results, logs, Timeline)."""
        return self._call_reduced(Timeline(_ngroups(len(cfgs), groups, ngroups), bins, bin_ms), cfgs, groups, want_logs)

    def run_trials_sojourn(self, cfgs, arrival_bins, arrival_bin_ms, delay_bins, delay_bin_ms, groups=None, want_logs=False, ngroups=None):
        """run_trials plus the histogram of the time from arrival to Msg4 by arrival row per trial group, reduced on the device from the per-UE log records
        the simulation kernels leave there (prach_run_trials_sojourn; Beta.c and RandomAccessWithNOMA trials only).  groups / ngroups / want_logs as in
        run_trials_dist.  Returns (results, logs, Sojourn)."""
        return self._call_reduced(Sojourn(_ngroups(len(cfgs), groups, ngroups), arrival_bins, arrival_bin_ms, delay_bins, delay_bin_ms), cfgs, groups, want_logs)

    def run_trials_xtab(self, cfgs, rows=("arrival", 500, 20), cols=("state", 1, 7), who=XTAB_WHO["all"], groups=None, want_logs=False, ngroups=None):
        """run_trials plus the outcome cross-tabulation per trial group — a table of two per-UE quantities (rows, cols: (field, width, bins), a field of
        XTAB_FIELD_NAMES) over the classes of UEs in ``who`` — reduced on the device from the per-UE log records the simulation kernels leave there
        (prach_run_trials_xtab; Beta.c and RandomAccessWithNOMA trials only).  The default: what became of the UEs by when they arrived.  groups / ngroups /
        want_logs as in run_trials_dist.  Returns (results, logs, Xtab)."""
        return self._call_reduced(Xtab(_ngroups(len(cfgs), groups, ngroups), rows, cols, who), cfgs, groups, want_logs)

    def run_trials_summary(self, cfgs, permille=(500, 950, 990), want_logs=False):
        """run_trials plus one summary row per trial — counts, sums, maxima and exact order statistics (levels in permille) of the sojourn, of `timer` and of
        the preamble transmissions over the trial's successful UEs — selected on the device (prach_run_trials_summary; Beta.c and RandomAccessWithNOMA
        trials only).  Returns (results, logs, Summary); Summary.stats() gives mean and spread across the trials."""
        return self._call_per_trial("prach_run_trials_summary", Summary(len(cfgs), permille), cfgs, want_logs)

    def run_trials_pick(self, cfgs, where=(), order="index", key=None, k=16, who=XTAB_WHO["all"], want_logs=False):
        """run_trials plus, per trial, the k UEs that match the clauses ``where`` ((field, lo, hi), a field of XTAB_FIELD_NAMES, lo <= value <= hi) among the
        classes ``who`` — the first k by UE index (order "index"), or the k with the "largest" / "smallest" value of the field ``key``, equal keys in ascending
        UE index — as records, and the exact number of matches, selected on the device (prach_run_trials_pick; Beta.c and RandomAccessWithNOMA trials only).
        Xtab.cell_clauses gives the ``where`` of a cell of a cross-tabulation.  Returns (results, logs, Pick)."""
        return self._call_per_trial("prach_run_trials_pick", Pick(len(cfgs), where, order, key, k, who), cfgs, want_logs)

    def run_trials_columns(self, cfgs, fields, device=False, want_logs=False):
        """run_trials plus the per-UE columns: for every UE of every trial the asked-for ``fields`` — names of XTAB_FIELD_NAMES, the menu of the
        cross-tabulation, -1 where undefined, or ``raw:NAME`` for a word of the log record as it is — as int32 columns computed on the device
        (prach_run_trials_columns; Beta.c and RandomAccessWithNOMA trials only).  device=False: Columns.data is a numpy array, 4 bytes per UE and field over
        the bus.  device=True: it is a torch tensor on this engine's GPU that the kernel wrote straight into (prach_run_trials_columns_device), and nothing
        but the headers crosses the bus; torch must have been imported BEFORE this package loaded its library, so that both use one HIP runtime.
        Returns (results, logs, Columns)."""
        return self._run_columns("run_trials_columns", "prach_run_trials_columns", cfgs, fields, device, want_logs, columns_spec, columns_header_dtype(), PrachColumns, Columns)

    def _run_columns(self, what, name, cfgs, fields, device, want_logs, make_spec, hdr_dtype, hdr_struct, cls):
        """What run_trials_columns and run_trials_noma_columns share: the spec, the headers, the host or torch destination (and the one-runtime guard)."""
        import numpy as np
        sp, ids = make_spec(fields)
        rows = sum(int(c.nUE) for c in cfgs)
        hdr = np.zeros(len(cfgs), dtype=hdr_dtype)
        hp = hdr.ctypes.data_as(C.POINTER(hdr_struct))
        if not device:
            data = np.empty((max(len(ids), 1), rows), dtype=np.int32)
            res, logs = self._call(name, cfgs, want_logs, C.byref(sp), hp, data.ctypes.data, rows)
            return res, logs, cls(ids, hdr, data[:len(ids)])
        lib()
        if _lib_before_torch:
            raise PrachError(-1, f"({what} device=True: libprach_hip.so was loaded before torch was imported, so torch brought a HIP runtime of its "
                                 "own and its device pointers mean nothing to the library's: import torch first, then make the first call into this package)")
        import torch
        if len(hip_runtimes()) > 1:
            raise PrachError(-1, f"({what} device=True: two HIP runtimes are loaded, {', '.join(hip_runtimes())}: torch and libprach_hip.so must share one)")
        data = torch.empty((max(len(ids), 1), rows), dtype=torch.int32, device=torch.device("cuda", self.device))
        torch.cuda.synchronize(self.device)  # (the engine's stream is not torch's)
        res, logs = self._call(name + "_device", cfgs, want_logs, C.byref(sp), hp, data.data_ptr(), rows)
        return res, logs, cls(ids, hdr, data[:len(ids)])

    def run_trials_noma_census(self, cfgs, rows=("arrival", 500, 20), cols=("state", 1, 9), who=NOMA_WHO["all"], groups=None, want_logs=False, ngroups=None):
        """run_trials plus the NOMA.c outcome census per trial group — a table of two quantities of the NOMA menu (rows, cols: (field, width, bins), a field of
        NOMA_FIELD_NAMES) over the classes of UEs in ``who`` — reduced on the device from the log records prach::noma_kernel leaves there
        (prach_run_trials_noma_census; NOMA.c trials with Philox only).  The default: what became of the UEs by when they arrived.  groups / ngroups /
        want_logs as in run_trials_dist.  Returns (results, logs, NomaCensus)."""
        return self._call_reduced(NomaCensus(_ngroups(len(cfgs), groups, ngroups), rows, cols, who), cfgs, groups, want_logs)

    def run_trials_noma_summary(self, cfgs, fields=("sojourn", "timer", "ptc", "lost"), who=NOMA_WHO["served"], permille=(500, 950, 990), want_logs=False):
        """run_trials plus one summary row per NOMA.c trial — the four class counts and, for up to four ``fields`` of NOMA_FIELD_NAMES over the UEs of the
        classes ``who`` whose value is defined, their number, sum, maximum and EXACT order statistics at the levels ``permille`` — selected on the device
        (prach_run_trials_noma_summary; NOMA.c trials with Philox only).  NomaSummary.stats gives the spread between the trials of a group.  Returns
        (results, logs, NomaSummary)."""
        return self._call_per_trial("prach_run_trials_noma_summary", NomaSummary(len(cfgs), fields, who, permille), cfgs, want_logs)

    def run_trials_noma_pick(self, cfgs, where=(), order="index", key=None, k=16, who=NOMA_WHO["all"], want_logs=False):
        """run_trials_pick for NOMA.c trials with Philox: clauses, key and ``who`` over the NOMA menu (fields of NOMA_FIELD_NAMES, classes of NOMA_WHO), selected
        on the device (prach_run_trials_noma_pick).  NomaCensus.cell_clauses gives the ``where`` of a census cell.  Returns (results, logs, NomaPick)."""
        return self._call_per_trial("prach_run_trials_noma_pick", NomaPick(len(cfgs), where, order, key, k, who), cfgs, want_logs)

    def run_trials_noma_columns(self, cfgs, fields, device=False, want_logs=False):
        """run_trials_columns for NOMA.c trials with Philox: ``fields`` are names of NOMA_FIELD_NAMES, -1 where undefined, or ``raw:NAME``
        (prach_run_trials_noma_columns, prach_run_trials_noma_columns_device).  device as in run_trials_columns.  Returns (results, logs, NomaColumns)."""
        return self._run_columns("run_trials_noma_columns", "prach_run_trials_noma_columns", cfgs, fields, device, want_logs, noma_columns_spec, noma_columns_header_dtype(),
                                 PrachNomaColumns, NomaColumns)

    def run_trials_noma_trace(self, cfgs, bins, bin_ms=5, groups=None, ngroups=None, want_logs=False):
        """run_trials plus NOMA.c's channel trace per trial group — per access slot and sector the preambles sent, the bins used and alone, the UEs granted, the
        power-domain pairs and the pairs that decoded one UE, by time — recorded by prach::noma_kernel while it runs and reduced on the device
        (prach_run_trials_noma_trace; NOMA.c trials with Philox only).  groups / ngroups / want_logs as in run_trials_dist.  Returns (results, logs, NomaTrace)."""
        return self._call_reduced(NomaTrace(_ngroups(len(cfgs), groups, ngroups), bins, bin_ms), cfgs, groups, want_logs)

    def run_trials_noma_timeline(self, cfgs, bins, bin_ms=5, groups=None, ngroups=None, want_logs=False):
        """run_trials plus NOMA.c's timeline per trial group and sector — arrivals, served, dropped, the sojourn and timer sums of the served by arrival time, and
        the completions by completion time, on the bins of run_trials_noma_trace — reduced on the device from the log records the simulation kernel leaves there
        (prach_run_trials_noma_timeline; NOMA.c trials with Philox only).  groups / ngroups / want_logs as in run_trials_dist.  Returns
        (results, logs, NomaTimeline)."""
        return self._call_reduced(NomaTimeline(_ngroups(len(cfgs), groups, ngroups), bins, bin_ms), cfgs, groups, want_logs)

    def run_trials_noma_gain(self, cfgs, bins=65, width=200, lo=-16200, groups=None, ngroups=None, want_logs=False):
        """run_trials plus NOMA.c's near-far profiles per trial group and sector — arrived, served, dropped, sojourn, lost-time and preamble-count sums by the
        UE's channel-gain level floor(1000 ln g) — reduced on the device from the log records and the launch's own activation table
        (prach_run_trials_noma_gain; NOMA.c trials with Philox only).  The defaults cover -162.00 ... -32.00 in 10 ln g, the whole range a trial can produce.
        groups / ngroups / want_logs as in run_trials_dist.  Returns (results, logs, NomaGain)."""
        return self._call_reduced(NomaGain(_ngroups(len(cfgs), groups, ngroups), bins, width, lo), cfgs, groups, want_logs)

    def run_trials_trace(self, cfgs, bins, bin_ms=1, groups=None, want_logs=False, ngroups=None):
        """run_trials plus the per-subframe preamble trace per trial group — preambles used (calls), decoded (singles) and what the subframes added to
        totalPreambleTxop and collisionPreambles, by time — recorded by the simulation kernels while they run and reduced on the device
        (prach_run_trials_trace; Beta.c and RandomAccessWithNOMA trials only).  groups / ngroups / want_logs as in run_trials_dist.  Returns
        (results, logs, Trace)."""
        return self._call_reduced(Trace(_ngroups(len(cfgs), groups, ngroups), bins, bin_ms), cfgs, groups, want_logs)

    @staticmethod
    def _log_buffers(cfgs, want_logs):
        n = len(cfgs)
        logs = [None] * n
        lp = None
        if want_logs:
            which = range(n) if want_logs is True else sorted(set(int(k) for k in want_logs))
            for k in which:
                logs[k] = (PrachUeLog * cfgs[k].nUE)()
            lp = (C.POINTER(PrachUeLog) * n)(*[C.cast(l, C.POINTER(PrachUeLog)) if l is not None else C.POINTER(PrachUeLog)()
                                               for l in logs])
        return logs, lp

    def device_glibc_stream(self, seed, first, n):
        import numpy as np
        out = np.empty(n, dtype=np.int32)
        rc = lib().prach_device_glibc_stream(self._h, seed, first, n, out.ctypes.data)
        if rc != OK:
            raise PrachError(rc, "(prach_device_glibc_stream)")
        return out

    def timing(self) -> PrachTiming:
        t = PrachTiming()
        lib().prach_last_timing(self._h, C.byref(t))
        return t


def arrival_schedule(cfg: PrachCfg):
    cap = 60000 // max(1, cfg.accessTime) + 2
    out = (C.c_int32 * cap)()
    na = C.c_int32(0)
    n = lib().prach_arrival_schedule(C.byref(cfg), out, cap, C.byref(na))
    return list(out[:n]), na.value


def glibc_stream(seed, first, n):
    import numpy as np
    out = np.empty(n, dtype=np.int32)
    lib().prach_glibc_stream(seed, first, n, out.ctypes.data)
    return out


def format_logs(logs, nUE) -> bytes:
    cap = nUE * 384 + 1  # a line is at most 378 bytes (prach_host.c): one formatting pass
    buf = C.create_string_buffer(cap)
    n = lib().prach_format_logs(logs, nUE, buf, cap)
    return buf.raw[:n]


def format_results(cfg, res, latency=0.0) -> bytes:
    buf = C.create_string_buffer(2048)
    n = lib().prach_format_results(C.byref(cfg), C.byref(res), latency, buf, 2048)
    return buf.raw[:n]


def format_stdout(cfg, res, latency=0.0) -> bytes:
    buf = C.create_string_buffer(4096)
    n = lib().prach_format_stdout(C.byref(cfg), C.byref(res), latency, buf, 4096)
    return buf.raw[:n]


def noma_activation_table(cfg: PrachCfg):
    """(preamble0, sector, gain, ln gain, draws) per UE of the NOMA.c variant (host side, no GPU)."""
    import numpy as np
    n = cfg.nUE
    pre0, sec = np.empty(n, np.int32), np.empty(n, np.int32)
    gain, lgain = np.empty(n, np.float64), np.empty(n, np.float64)
    nd = np.empty(n, np.uint32)
    rc = lib().prach_noma_activation_table(C.byref(cfg), pre0.ctypes.data, sec.ctypes.data, gain.ctypes.data, lgain.ctypes.data, nd.ctypes.data)
    if rc != OK:
        raise PrachError(rc, "(prach_noma_activation_table)")
    return pre0, sec, gain, lgain, nd


def noma_activation_table_device(engine, cfg: PrachCfg):
    """The same table as the engine builds it on the GPU (Philox mode) + a per-UE flag: recomputed on the host (see include/prach.h)."""
    import numpy as np
    n = cfg.nUE
    pre0, sec = np.empty(n, np.int32), np.empty(n, np.int32)
    gain, lgain = np.empty(n, np.float64), np.empty(n, np.float64)
    nd, flagged = np.empty(n, np.uint32), np.empty(n, np.uint8)
    rc = lib().prach_noma_activation_table_device(engine._h, C.byref(cfg), pre0.ctypes.data, sec.ctypes.data, gain.ctypes.data, lgain.ctypes.data,
                                                  nd.ctypes.data, flagged.ctypes.data)
    if rc != OK:
        raise PrachError(rc, "(prach_noma_activation_table_device)")
    return pre0, sec, gain, lgain, nd, flagged


def format_noma_line(cfg, res) -> bytes:
    buf = C.create_string_buffer(256)
    n = lib().prach_format_noma_line(C.byref(cfg), C.byref(res), buf, 256)
    return buf.raw[:n]


def results_csv(rows_of_results_texts):
    """results.csv bytes for [[Results.txt text of seed 0, seed 1, ...] per nUE point] (AveragePerformance.py)."""
    out = b""
    for texts in rows_of_results_texts:
        acc = (C.c_double * 6)()
        for t in texts:
            rc = lib().prach_results_csv_accumulate(acc, t if isinstance(t, bytes) else t.encode())
            if rc != OK:
                raise PrachError(rc, "(prach_results_csv_accumulate)")
        buf = C.create_string_buffer(512)
        n = lib().prach_results_csv_row(acc, len(texts), buf, 512)
        out += buf.raw[:n]
    return out


def dist_tile_ues() -> int:
    return lib().prach_dist_tile_ues()


def _ngroups(n, groups, ngroups):
    """The number of groups of n trials: as given, or one per trial without a group table, or the largest group id + 1."""
    return ngroups if ngroups is not None else n if groups is None else int(max(groups)) + 1


def _log_ptr(lg):
    """One trial's per-UE log — a ctypes array of PrachUeLog or an int32 array of shape [nUE, 16] — as (pointer, nUE, what keeps the memory alive)."""
    import numpy as np
    if isinstance(lg, np.ndarray):
        a = np.ascontiguousarray(lg, dtype=np.int32).reshape(-1, 16)
        return a.ctypes.data_as(C.POINTER(PrachUeLog)), a.shape[0], a
    return C.cast(lg, C.POINTER(PrachUeLog)), len(lg), lg


def _from_logs(red, logs, groups, cfgs=None, steps=None):
    """Adds every log to its group of `red` with the kind's host-side definition, prach_<kind>_accumulate_logs, which takes the trial's config (if cfgs) and
    the subframes it ran (if steps) in front of the log."""
    name = f"prach_{red._KIND}_accumulate_logs"
    sp = red.spec()
    for k, lg in enumerate(logs):
        g = k if groups is None else int(groups[k])
        ptr, nue, _keep = _log_ptr(lg)
        d = red._group(g)
        more = ([C.byref(cfgs[k])] if cfgs is not None else []) + ([int(steps[k])] if steps is not None else [])
        rc = getattr(lib(), name)(C.byref(sp), *more, ptr, nue, C.byref(d), *red._ptrs(red._RUN, g))
        if rc != OK:
            raise PrachError(rc, f"({name})")
        red._store(g, d)
    return red


def dist_from_logs(logs, delay_bins, delay_bin_ms=1, groups=None, ngroups=None) -> Dist:
    """The host-side definition of the distributions (prach_dist_accumulate_logs): logs[k] is one trial's per-UE log — a ctypes array of PrachUeLog
    or an int32 array of shape [nUE, 16] — added to group groups[k] (None: group k)."""
    return Dist.from_logs(logs, delay_bins, delay_bin_ms, groups=groups, ngroups=ngroups)


def dist_quantile(dist: Dist, g: int, q: float) -> int:
    """Lower edge (ms) of the delay bin holding the ceil(q * success)-th smallest delay of group g; -1: no successful UE, or in the overflow."""
    sp, d = dist.spec(), dist._group(g)
    return int(lib().prach_dist_delay_quantile(C.byref(sp), C.byref(d), dist._hists(g)[0], q))


def dist_csv(dist: Dist, labels=None) -> bytes:
    """The CSV text of every group (prach_dist_format_csv), labelled labels[g] (default: the group number)."""
    return dist.csv(labels)


def timeline_tile_ues() -> int:
    return lib().prach_timeline_tile_ues()


def timeline_window_bins() -> int:
    return lib().prach_timeline_window_bins()


def timeline_from_logs(cfgs, logs, bins, bin_ms=1, groups=None, ngroups=None) -> Timeline:
    """The host-side definition of the timelines (prach_timeline_accumulate_logs): logs[k] is the per-UE log of the trial with config cfgs[k] — a ctypes
    array of PrachUeLog or an int32 array of shape [nUE, 16] — added to group groups[k] (None: group k)."""
    return Timeline.from_logs(logs, bins, bin_ms, cfgs=cfgs, groups=groups, ngroups=ngroups)


def timeline_csv(tl: Timeline, labels=None) -> bytes:
    """The CSV text of every group (prach_timeline_format_csv), labelled labels[g] (default: the group number)."""
    return tl.csv(labels)


def sojourn_tile_ues() -> int:
    return lib().prach_sojourn_tile_ues()


def sojourn_window_words() -> int:
    return lib().prach_sojourn_window_words()


def sojourn_from_logs(cfgs, logs, arrival_bins, arrival_bin_ms, delay_bins, delay_bin_ms, groups=None, ngroups=None) -> Sojourn:
    """The host-side definition of the sojourn histograms (prach_sojourn_accumulate_logs): logs[k] is the per-UE log of the trial with config cfgs[k] — a
    ctypes array of PrachUeLog or an int32 array of shape [nUE, 16] — added to group groups[k] (None: group k)."""
    return Sojourn.from_logs(logs, arrival_bins, arrival_bin_ms, delay_bins, delay_bin_ms, cfgs=cfgs, groups=groups, ngroups=ngroups)


def sojourn_csv(sj: Sojourn, labels=None) -> bytes:
    """The CSV text of every group (prach_sojourn_format_csv), labelled labels[g] (default: the group number)."""
    return sj.csv(labels)


def trace_tile_subframes() -> int:
    return lib().prach_trace_tile_subframes()


def trace_csv(tr: Trace, labels=None) -> bytes:
    """The CSV text of every group (prach_trace_format_csv), labelled labels[g] (default: the group number)."""
    return tr.csv(labels)


def noma_trace_tile_rows() -> int:
    return lib().prach_noma_trace_tile_rows()


def noma_timeline_tile_ues() -> int:
    return lib().prach_noma_timeline_tile_ues()


def noma_timeline_window_bins() -> int:
    return lib().prach_noma_timeline_window_bins()


def noma_gain_tile_ues() -> int:
    return lib().prach_noma_gain_tile_ues()


def noma_gain_lds_max_bins() -> int:
    return lib().prach_noma_gain_lds_max_bins()


def noma_gain_level(lgain: float) -> int:
    """The gain level of ln(gain): floor(1000 * lgain), NOMA_GAIN_NO_LEVEL where there is none (prach_noma_gain_level)."""
    return int(lib().prach_noma_gain_level(float(lgain)))


def noma_gain_levels(cfg):
    """The host's gain levels of every UE of a NOMA.c Philox trial, as an int32 array [nUE] (prach_noma_gain_levels): joins with run_trials_noma_columns."""
    import numpy as np
    out = np.empty(max(int(cfg.nUE), 0), dtype=np.int32)
    rc = lib().prach_noma_gain_levels(C.byref(cfg), out.ctypes.data_as(C.c_void_p))
    if rc != OK:
        raise PrachError(rc, "(prach_noma_gain_levels)")
    return out


def noma_gain_from_logs(cfgs, steps, logs, bins=65, width=200, lo=-16200, groups=None, ngroups=None) -> NomaGain:
    """The host-side definition of the near-far profiles with the host's own levels (prach_noma_gain_accumulate_logs): logs[k] is the per-UE log of the NOMA.c
    Philox trial with config cfgs[k] that ran steps[k] subframes — a ctypes array of PrachUeLog or an int32 array [nUE, 16] — added to group groups[k]."""
    return NomaGain.from_logs(logs, bins, width, lo, cfgs=cfgs, steps=steps, groups=groups, ngroups=ngroups)


def noma_gain_from_levels(cfgs, steps, logs, levels, bins=65, width=200, lo=-16200, groups=None, ngroups=None) -> NomaGain:
    """THE DEFINITION with the levels as given (prach_noma_gain_accumulate_levels; any RNG mode): levels[k] is an int32 array [nUE] next to logs[k]."""
    import numpy as np
    red = NomaGain(_ngroups(len(logs), groups, ngroups), bins, width, lo)
    sp = red.spec()
    for k, lg in enumerate(logs):
        g = k if groups is None else int(groups[k])
        ptr, nue, _keep = _log_ptr(lg)
        lv = np.ascontiguousarray(levels[k], dtype=np.int32)
        if lv.shape != (nue,):
            raise ValueError("one level per UE of the log")
        d = red._group(g)
        rc = lib().prach_noma_gain_accumulate_levels(C.byref(sp), C.byref(cfgs[k]), int(steps[k]), ptr, nue, lv.ctypes.data_as(C.c_void_p), C.byref(d), *red._ptrs("array", g))
        if rc != OK:
            raise PrachError(rc, "(prach_noma_gain_accumulate_levels)")
        red._store(g, d)
    return red


def noma_gain_csv(gn: NomaGain, labels=None) -> bytes:
    """The CSV text of every group (prach_noma_gain_format_csv), labelled labels[g] (default: the group number)."""
    return gn.csv(labels)


def noma_timeline_from_logs(cfgs, steps, logs, bins, bin_ms=5, groups=None, ngroups=None) -> NomaTimeline:
    """The host-side definition of the NOMA timelines (prach_noma_timeline_accumulate_logs): logs[k] is the per-UE log of the NOMA.c trial with config cfgs[k] that
    ran steps[k] subframes (prach_result.steps) — a ctypes array of PrachUeLog or an int32 array of shape [nUE, 16] — added to group groups[k] (None: group k)."""
    return NomaTimeline.from_logs(logs, bins, bin_ms, cfgs=cfgs, steps=steps, groups=groups, ngroups=ngroups)


def noma_timeline_csv(tl: NomaTimeline, labels=None) -> bytes:
    """The CSV text of every group (prach_noma_timeline_format_csv), labelled labels[g] (default: the group number)."""
    return tl.csv(labels)


def noma_trace_csv(tr: NomaTrace, labels=None) -> bytes:
    """The CSV text of every group (prach_noma_trace_format_csv), labelled labels[g] (default: the group number)."""
    return tr.csv(labels)


def summary_max_value() -> int:
    return lib().prach_summary_max_value()


def summary_from_logs(cfgs, logs, permille=(500, 950, 990)) -> Summary:
    """The host-side definition of the per-trial summary (prach_summary_from_logs): row k from logs[k], the per-UE log of the trial with config cfgs[k] — a
    ctypes array of PrachUeLog or an int32 array of shape [nUE, 16]."""
    sm = Summary(len(logs), permille)
    sp = sm.spec()
    rows = sm._rows_ptr()
    for k, lg in enumerate(logs):
        ptr, nue, _keep = _log_ptr(lg)
        rc = lib().prach_summary_from_logs(C.byref(sp), C.byref(cfgs[k]), ptr, nue, C.byref(rows[k]))
        if rc != OK:
            raise PrachError(rc, "(prach_summary_from_logs)")
    return sm


def summary_csv(sm: Summary, groups=None, ngroups=None, labels=None) -> bytes:
    """The CSV text of the statistics of every group of trials (prach_summary_stats, prach_summary_format_csv), labelled labels[g] (default: the group
    number): `label,metric,n,mean,sd,sem,min,max`."""
    fmt = getattr(lib(), sm._FORMAT_CSV)
    st = sm.stats(groups, ngroups)
    sp = sm.spec()
    out = b""
    for g in range(st.shape[0]):
        args = (C.byref(sp), st[g].ctypes.data_as(C.POINTER(PrachStat)), str(g if labels is None else labels[g]).encode())
        need = fmt(*args, None, 0)
        buf = C.create_string_buffer(need + 1)
        n = fmt(*args, buf, need + 1)
        out += buf.raw[:n]
    return out


def noma_summary_from_logs(cfgs, steps, logs, fields=("sojourn", "timer", "ptc", "lost"), who=NOMA_WHO["served"], permille=(500, 950, 990)) -> NomaSummary:
    """The host-side definition of the NOMA summary (prach_noma_summary_from_logs): row k from logs[k], the per-UE log of the NOMA.c trial with config cfgs[k]
    that ran steps[k] subframes (prach_result.steps) — a ctypes array of PrachUeLog or an int32 array of shape [nUE, 16].  Both RNG modes."""
    sm = NomaSummary(len(logs), fields, who, permille)
    sp = sm.spec()
    rows = sm._rows_ptr()
    for k, lg in enumerate(logs):
        ptr, nue, _keep = _log_ptr(lg)
        rc = lib().prach_noma_summary_from_logs(C.byref(sp), C.byref(cfgs[k]), int(steps[k]), ptr, nue, C.byref(rows[k]))
        if rc != OK:
            raise PrachError(rc, "(prach_noma_summary_from_logs)")
    return sm


def noma_summary_csv(sm: NomaSummary, groups=None, ngroups=None, labels=None) -> bytes:
    """The CSV text of the statistics of every group of trials (prach_noma_summary_stats, prach_noma_summary_format_csv), labelled labels[g] (default: the
    group number): `label,metric,n,mean,sd,sem,min,max`."""
    return summary_csv(sm, groups, ngroups, labels)


def _pick_from_logs(fn, pk, cfgs, steps, logs):
    sp = pk.spec()
    hdr = pk._headers_ptr()
    for t, lg in enumerate(logs):
        ptr, nue, _keep = _log_ptr(lg)
        rc = getattr(lib(), fn)(C.byref(sp), C.byref(cfgs[t]), int(steps[t]), ptr, nue, C.byref(hdr[t]), pk._rows_ptr(t))
        if rc != OK:
            raise PrachError(rc, f"({fn})")
    return pk


def pick_from_logs(cfgs, steps, logs, where=(), order="index", key=None, k=16, who=XTAB_WHO["all"]) -> Pick:
    """The host-side definition of the pick (prach_pick_from_logs): trial t from logs[t], the per-UE log of the trial with config cfgs[t] that ran steps[t]
    subframes (prach_result.steps) — a ctypes array of PrachUeLog, as Engine.run_trials returns it, or an int32 array of shape [nUE, 16]."""
    return _pick_from_logs("prach_pick_from_logs", Pick(len(logs), where, order, key, k, who), cfgs, steps, logs)


def noma_pick_from_logs(cfgs, steps, logs, where=(), order="index", key=None, k=16, who=NOMA_WHO["all"]) -> NomaPick:
    """The host-side definition of the NOMA pick (prach_noma_pick_from_logs), as pick_from_logs: NOMA.c trials, both RNG modes."""
    return _pick_from_logs("prach_noma_pick_from_logs", NomaPick(len(logs), where, order, key, k, who), cfgs, steps, logs)


def noma_pick_csv(pk: NomaPick, cfgs=None, labels=None) -> bytes:
    """pick_csv for a NOMA pick (prach_noma_pick_format_csv: the same lines)."""
    return pick_csv(pk, cfgs, labels, _fn="prach_noma_pick_format_csv")


def pick_csv(pk: Pick, cfgs=None, labels=None, _fn="prach_pick_format_csv") -> bytes:
    """The CSV text of every trial's pick (prach_pick_format_csv), trial by trial: labelled labels[t] (default: the trial's nUE), with the seed of cfgs[t]
    (default 0)."""
    fmt = getattr(lib(), _fn)
    out = []
    sp = pk.spec()
    hdr = pk._headers_ptr()
    for t in range(len(pk.headers)):
        label = str(int(pk.headers["nUE"][t]) if labels is None else labels[t]).encode()
        args = (C.byref(sp), C.byref(hdr[t]), pk._rows_ptr(t), label, t, int(cfgs[t].seed) if cfgs is not None else 0)
        need = fmt(*args, None, 0)
        buf = C.create_string_buffer(need + 1)
        n = fmt(*args, buf, need + 1)
        assert n == need
        out.append(buf.raw[:n])
    return b"".join(out)


def xtab_tile_ues() -> int:
    return lib().prach_xtab_tile_ues()


def xtab_window_words() -> int:
    return lib().prach_xtab_window_words()


def xtab_from_logs(cfgs, steps, logs, rows=("arrival", 500, 20), cols=("state", 1, 7), who=XTAB_WHO["all"], groups=None, ngroups=None) -> Xtab:
    """The host-side definition of the cross-tabulation (prach_xtab_accumulate_logs): logs[k] is the per-UE log of the trial with config cfgs[k] that ran
    steps[k] subframes (prach_result.steps) — a ctypes array of PrachUeLog or an int32 array of shape [nUE, 16] — added to group groups[k] (None: group k)."""
    return Xtab.from_logs(logs, rows, cols, who, cfgs=cfgs, steps=steps, groups=groups, ngroups=ngroups)


def xtab_csv(xt: Xtab, labels=None) -> bytes:
    """The CSV text of every group (prach_xtab_format_csv), labelled labels[g] (default: the group number)."""
    return xt.csv(labels)


def columns_tile_ues() -> int:
    return lib().prach_columns_tile_ues()


def _columns_from_logs(name, make_spec, hdr_dtype, classes, cls, cfgs, steps, logs, fields):
    """What columns_from_logs and noma_columns_from_logs share.  classes: the headers' class counts in the order of the menu's STATE values, the last one taking
    every state from its own on."""
    import numpy as np
    sp, ids = make_spec(fields)
    state, _ = make_spec(["state"])
    hdr = np.zeros(len(logs), dtype=hdr_dtype)
    ptrs = [_log_ptr(lg) for lg in logs]
    hdr["nUE"] = [nue for _, nue, _ in ptrs]
    hdr["offset"] = np.concatenate([[0], np.cumsum(hdr["nUE"], dtype=np.uint64)[:-1]]) if len(logs) else []
    rows = int(hdr["nUE"].sum())
    data = np.empty((max(len(ids), 1), rows), dtype=np.int32)
    for k, (ptr, nue, _keep) in enumerate(ptrs):
        st = np.empty(nue, dtype=np.int32)
        for spec, out, stride in ((sp, data.ctypes.data + 4 * int(hdr["offset"][k]), rows), (state, st.ctypes.data, nue)):
            rc = getattr(lib(), name)(C.byref(spec), C.byref(cfgs[k]), int(steps[k]), ptr, nue, out, stride)
            if rc != OK:
                raise PrachError(rc, f"({name})")
        for v, c in enumerate(classes):
            hdr[c][k] = (st == v).sum() if v < len(classes) - 1 else (st >= v).sum()
    return cls(ids, hdr, data[:len(ids)])


def columns_from_logs(cfgs, steps, logs, fields) -> Columns:
    """The host-side definition of the columns (prach_columns_from_logs): trial k from logs[k], the per-UE log of the trial with config cfgs[k] that ran
    steps[k] subframes (prach_result.steps) — a ctypes array of PrachUeLog, as Engine.run_trials returns it, or an int32 array of shape [nUE, 16].  The class
    counts of the headers are those of the definition's own STATE column."""
    return _columns_from_logs("prach_columns_from_logs", columns_spec, columns_header_dtype(), ("idle", "served", "unserved"), Columns, cfgs, steps, logs, fields)


def noma_census_tile_ues() -> int:
    return lib().prach_noma_census_tile_ues()


def noma_census_from_logs(cfgs, steps, logs, rows=("arrival", 500, 20), cols=("state", 1, 9), who=NOMA_WHO["all"], groups=None, ngroups=None) -> NomaCensus:
    """The host-side definition of the NOMA census (prach_noma_census_accumulate_logs): logs[k] is the per-UE log of the NOMA.c trial with config cfgs[k] that
    ran steps[k] subframes (prach_result.steps) — a ctypes array of PrachUeLog or an int32 array of shape [nUE, 16] — added to group groups[k] (None: group k)."""
    return NomaCensus.from_logs(logs, rows, cols, who, cfgs=cfgs, steps=steps, groups=groups, ngroups=ngroups)


def noma_census_csv(cs: NomaCensus, labels=None) -> bytes:
    """The CSV text of every group (prach_noma_census_format_csv: the lines of xtab_csv), labelled labels[g] (default: the group number)."""
    return cs.csv(labels)


def noma_columns_from_logs(cfgs, steps, logs, fields) -> NomaColumns:
    """The host-side definition of the NOMA columns (prach_noma_columns_from_logs), as columns_from_logs.  The class counts of the headers are those of the
    definition's own STATE column."""
    return _columns_from_logs("prach_noma_columns_from_logs", noma_columns_spec, noma_columns_header_dtype(), ("idle", "served", "dropped", "pending"), NomaColumns, cfgs, steps,
                              logs, fields)
