#!/usr/bin/env python3
"""The batched call (ek_hip_eigenpairs_batched_device) against the only other way to solve many small problems: a host
loop over ek_hip_solve_device.  Device-resident arrays both ways, one process (tools, not product).

  python tools/batched_timing.py [--sizes 30,64,128] [--batches 1,256,4096] [--loop-max 64]
  python tools/batched_timing.py --once 64g      one batched call (256 generalized pairs of order 64 with vectors)
                                                 after a warm-up: what a kernel trace should look at

Per (problem, jobz, n, batch): one warm-up of each kind, then three rounds that alternate the kinds, best by wall clock
(both calls synchronise; both work in place, so the inputs are restored outside the clock).  The loop is timed over
min(batch, --loop-max) pairs and scaled to the batch.  "device" is the launch's own time (events around it)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eigenkernel_amd import solver  # noqa: E402


def pairs(seed, count, n):
    """count well-conditioned pairs (A symmetric, B SPD with condition 10), column-major per problem."""
    rng = np.random.default_rng(seed)
    A = np.empty((count, n, n))
    B = np.empty((count, n, n))
    d = np.logspace(0.0, 1.0, n) if n > 1 else np.array([10.0])
    for b in range(count):
        G = rng.standard_normal((n, n))
        A[b] = (G + G.T) / 2.0
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        M = (Q * d) @ Q.T
        B[b] = (M + M.T) / 2.0
    return A, B


class Case:
    def __init__(self, lib, n, batch, distinct=64):
        self.lib, self.n, self.batch = lib, n, batch
        A, B = pairs(n, min(batch, distinct), n)
        reps = -(-batch // A.shape[0])
        self.hA = np.ascontiguousarray(np.tile(A, (reps, 1, 1))[:batch]).ravel()
        self.hB = np.ascontiguousarray(np.tile(B, (reps, 1, 1))[:batch]).ravel()
        self.keep = []
        self.dA, self.dB, self.dZ = (self.alloc(batch * n * n * 8) for _ in range(3))
        self.dw = self.alloc(batch * n * 8)
        self.info = np.zeros(batch, dtype=np.int32)

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.lib.ek_hip_malloc(ctypes.byref(p), int(nbytes)) == 0
        self.keep.append(p)
        return p

    def restore(self):
        assert self.lib.ek_hip_memcpy_h2d(self.dA, self.hA.ctypes.data, self.hA.nbytes) == 0
        assert self.lib.ek_hip_memcpy_h2d(self.dB, self.hB.ctypes.data, self.hB.nbytes) == 0

    def batched(self, problem, jobz):
        n, nn = self.n, self.n * self.n
        self.restore()
        sec = ctypes.c_double(0.0)
        t0 = time.perf_counter()
        rc = self.lib.ek_hip_eigenpairs_batched_device(problem, jobz, n, self.batch, self.dA, n, nn,
                                                       self.dB if problem else None, n, nn, self.dw,
                                                       self.dZ if jobz else None, n, nn,
                                                       self.info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                       ctypes.byref(sec))
        t = time.perf_counter() - t0
        assert rc == 0 and not self.info.any(), (rc, self.info[self.info != 0][:4])
        return t, sec.value

    def loop(self, problem, jobz, count):
        n, nn = self.n, self.n * self.n
        self.restore()
        at = lambda p, b, per: ctypes.c_void_p(p.value + b * per * 8)  # noqa: E731
        t0 = time.perf_counter()
        for b in range(count):
            if jobz:
                rc = self.lib.ek_hip_solve_device(problem, n, n, at(self.dA, b, nn), n,
                                                  at(self.dB, b, nn) if problem else None, n, at(self.dw, b, n),
                                                  at(self.dZ, b, nn), n, None, 0)
            else:
                rc = self.lib.ek_hip_eigenvalues_device(problem, n, 1, n, at(self.dA, b, nn), n,
                                                        at(self.dB, b, nn) if problem else None, n, at(self.dw, b, n),
                                                        None, 0)
            assert rc == 0, rc
        return (time.perf_counter() - t0) * (self.batch / count)

    def close(self):
        for p in self.keep:
            self.lib.ek_hip_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30,64,128")
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--loop-max", type=int, default=64)
    ap.add_argument("--once", default=None, help="<n>g or <n>s: one generalized / standard batch of 256 with vectors")
    args = ap.parse_args()
    lib = solver.load_library()
    assert lib.ek_hip_init(0) == 0
    if args.once:
        n, problem = int(args.once[:-1]), 1 if args.once.endswith("g") else 0
        c = Case(lib, n, 256)
        c.batched(problem, 1)
        t, dev = c.batched(problem, 1)
        print("once: n=%d problem=%d batch=256 wall %.3f ms device %.3f ms" % (n, problem, t * 1e3, dev * 1e3))
        c.close()
        lib.ek_hip_finalize()
        return
    print("# problem jobz     n batch | batched wall ms  device ms  us/problem  problems/s | loop ms (scaled)  "
          "us/problem | ratio")
    for n in (int(x) for x in args.sizes.split(",")):
        for batch in (int(x) for x in args.batches.split(",")):
            c = Case(lib, n, batch)
            count = min(batch, args.loop_max)
            for problem in (1, 0):
                for jobz in (1, 0):
                    tb, tl, dev = [], [], []
                    c.batched(problem, jobz); c.loop(problem, jobz, count)          # warm-up
                    for _ in range(3):
                        t, d = c.batched(problem, jobz)
                        tb.append(t); dev.append(d)
                        tl.append(c.loop(problem, jobz, count))
                    b, lo = min(tb), min(tl)
                    print("  %7d %4d %5d %5d | %15.3f %10.3f %11.2f %11.0f | %16.2f %11.1f | %6.1f"
                          % (problem, jobz, n, batch, b * 1e3, min(dev) * 1e3, b / batch * 1e6, batch / b, lo * 1e3,
                             lo / batch * 1e6, lo / b), flush=True)
            c.close()
    lib.ek_hip_finalize()


if __name__ == "__main__":
    main()
