"""The Python side every off-trial harness test shares (tests/tools/HARNESS.md): compiling a tests/tools/gpu_*_harness.hip, writing a job case file,
running one child under a time limit of its own, and the latch that stops a test file from starting further children after one ended abnormally.
The *_cases.py modules keep their cases, references and result layouts.  No GPU use and no package import here."""
import contextlib
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17")


class Abnormal(RuntimeError):
    """A child that exited non-zero, was signalled or ran into its time limit."""


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build(src, out_dir, flags=(), name=None):
    """Compiles tests/tools/<src> (host program + its kernels for gfx950) into out_dir; returns the executable's path."""
    exe = os.path.join(str(out_dir), name or os.path.splitext(src)[0])
    subprocess.check_call([hipcc(), *FLAGS, *flags, os.path.join(HERE, src), "-o", exe])
    return exe


def run(exe, args, timeout=120, ok=(0,)):
    """One child process, started as `timeout -k 10 <timeout> exe args...` with subprocess's own limit 30 s above it.  Raises Abnormal on an exit status
    outside `ok`, a signal or a timeout: the caller starts nothing more on the device.  Returns the finished process."""
    cmd = ["timeout", "-k", "10", str(timeout), str(exe), *map(str, args)]
    what = " ".join([os.path.basename(str(exe)), *(os.path.basename(str(a)) for a in args)])
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout + 30)
    except subprocess.TimeoutExpired as e:
        raise Abnormal(f"{what}: no end after {timeout + 30} s: {str(e.stderr or '')[-2000:]}") from e
    if p.returncode not in ok:
        raise Abnormal(f"{what}: exit {p.returncode}: {p.stderr[-2000:]}")
    return p


def constants(exe, parse=int):
    """`exe --constants` as {name: value}; no device is needed."""
    return {k: parse(v) for k, v in (line.split() for line in run(exe, ["--constants"], timeout=60).stdout.splitlines())}


def write_job_case(path, head, rows, arrays):
    """The case file of the job harnesses: header words, 8-int job rows, then every job's arrays in job order, all as little-endian int32."""
    with open(path, "wb") as f:
        for p in (head, rows, *arrays):
            f.write(np.ascontiguousarray(p, dtype="<i4").tobytes())


def log_jobs(jobs, words):
    """(rows, arrays) of log-record jobs: a row is nUE, words(k, job)[0], 0, accessTime, nslots, words(k, job)[1:] ...; the arrays logs[nUE][16], sched[nslots]."""
    rows = np.zeros((len(jobs), 8), dtype=np.int32)
    arrays = []
    for k, j in enumerate(jobs):
        group, *more = words(k, j)
        rows[k, :5 + len(more)] = [j.nue, group, 0, j.access_time, len(j.sched), *more]
        arrays += [j.logs.reshape(-1), j.sched]
    return rows, arrays


class Latch:
    """One per test file.  `with latch.child(what): ...` around every start of a child; after one raised Abnormal, guard() — and with it every later
    child() of the file — fails before anything is started."""

    def __init__(self):
        self.abnormal = []

    def guard(self):
        assert not self.abnormal, f"not started: {self.abnormal[0]}"

    def trip(self, what):
        self.abnormal.append(what)

    @contextlib.contextmanager
    def child(self, what):
        self.guard()
        try:
            yield
        except (Abnormal, subprocess.TimeoutExpired) as e:
            self.trip(f"{what}: {e}")
            raise

    def python_child(self, what, cmd, limit, env=None):
        """A Python child that drives the package itself, as `timeout -k 10 <limit> cmd...`.  Exit status 1 means "trials differ": the child ended on its
        own.  Any other non-zero status, or `run ended` in its output (a failed call may have been a device error), trips the latch; so does a timeout,
        which is raised.  Returns the finished process: the caller asserts on it."""
        self.guard()
        try:
            p = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], env=env, capture_output=True, text=True, timeout=limit + 30)
        except subprocess.TimeoutExpired as e:
            self.trip(f"{what}: {e}")
            raise
        if p.returncode not in (0, 1) or "run ended" in p.stdout:
            self.trip(f"{what}: exit status {p.returncode}: {p.stdout[-300:]}")
        return p
