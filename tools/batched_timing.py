#!/usr/bin/env python3
"""The batched call (ek_hip_eigenpairs_batched_device) against the only other way to solve many small problems: a host
loop over ek_hip_solve_device.  Device-resident arrays both ways, one process (tools, not product).

  python tools/batched_timing.py [--sizes 30,64,128] [--batches 1,256,4096] [--loop-max 64] [--itype 1]
                                                 --itype 2 / 3: the generalized rows solve A B x = l x / B A x = l x
                                                 through ek_hip_sygv_batched_device (the loop stays type 1's: a yardstick)
                                                 sizes above 128 (up to 256) time ek_hip_eigenpairs_xbatched_device
                                                 (--itype 2 / 3: ek_hip_sygv_xbatched_device) against the same host loop;
                                                 sizes above 256 (up to 512) ek_hip_eigenpairs_ybatched_device
                                                 (ek_hip_sygv_ybatched_device); --check, --window and --mixed stop at 256
  python tools/batched_timing.py --once 64g      one batched call (256 generalized pairs of order 64 with vectors)
                                                 after a warm-up: what a kernel trace should look at
  python tools/batched_timing.py --mixed [--mixed-batch 2048] [--mixed-orders 8,128]
                                                 problems of different orders: one variable call
                                                 (ek_hip_eigenpairs_vbatched_device, a stream per class and one stream)
                                                 against a uniform call per distinct order and against one uniform call
                                                 with every problem padded to order 128
  python tools/batched_timing.py --mixed --mixed-batch 512 --mixed-orders 129,256   (or 8,256)
                                                 an upper order above 128: the variable call is
                                                 ek_hip_eigenpairs_xvbatched_device, the baselines go through
                                                 ek_hip_eigenpairs_xbatched_device, the padding is to order 256, and the
                                                 class times are those of the classes of 256 / 128 / 64 / 32
  python tools/batched_timing.py --mixed --check --mixed-batch 512 --mixed-orders 129,256   (or 8,256)
                                                 the variable acceptance check (ek_hip_check_xvbatched_device;
                                                 ek_hip_check_vbatched_device up to order 128) on the variable solve's w
                                                 and Z, against one uniform check call per distinct order and against the
                                                 solve's device time; the classes' times and counts of the check
  python tools/batched_timing.py --check [--sizes 64,128] [--batches 1024,4096]
                                                 with vectors only: after each timed solve, the batched check
                                                 (ek_hip_check_batched_device; ek_hip_check_xbatched_device for sizes
                                                 above 128) on its w and Z -- the check's device time
                                                 beside the solve's, the worst res_max and orthogonality of the batch
                                                 --itype 2 / 3: the generalized rows time the type's own check
                                                 (ek_hip_check_sygv_batched_device; ek_hip_check_sygv_xbatched_device
                                                 above 128) behind the type's own solve
  python tools/batched_timing.py --once 64g --once-batch 1024 --check
                                                 one solve and one check after a warm-up of each
  python tools/batched_timing.py --window 0.125,1 [--sizes 64,128] [--batches 512,1024]
                                                 a window of that fraction of n (ek_hip_eigenpairs_window_batched_device; sizes
                                                 above 128: ek_hip_eigenpairs_window_xbatched_device)
                                                 by index and by value, with and without vectors, against the existing
                                                 call, the kinds alternated; then a fully clustered standard batch
                                                 (all_equal, two_clusters of tests/batched_cases.py) both ways
  python tools/batched_timing.py --window 0.125,1 --itype 2 [--sizes 64,128,256] [--batches 256]
                                                 the window call of type 2 / 3 (ek_hip_sygv_window_batched_device; above
                                                 128: ek_hip_sygv_window_xbatched_device) against the full call of the same
                                                 type and against the type-1 window call
  python tools/batched_timing.py --window 0.125 --check [--sizes 128,129,256] [--batches 256] [--itype 2]
                                                 the window check (ek_hip_check_window_xbatched_device) on the m, w and Z
                                                 of the window solve, against the full check of the same batch
                                                 (ek_hip_check_xbatched_device on all n columns of a full solve) and
                                                 against a host loop over ek_hip_check_sygvx_device, the kinds alternated;
                                                 --itype 2 / 3: ek_hip_check_sygv_window_xbatched_device behind the type's
                                                 window solve, against the type's full check and the type's host loop

  python tools/batched_timing.py --mixed --window 0.125 [--mixed-batch 512] [--mixed-orders 8,256] [--itype 1]
                                                 the variable-order window call (ek_hip_eigenpairs_window_xvbatched_device;
                                                 --itype 2 / 3: ek_hip_sygv_window_xvbatched_device), the lowest
                                                 max(1, fraction n[b]) pairs of every problem with vectors, against a
                                                 uniform window call per distinct order, the full variable call
                                                 (ek_hip_*_xvbatched_device) and one uniform window call with every
                                                 problem padded to the largest order; device times, a stream per class
                                                 and one stream, the classes' times and counts
  python tools/batched_timing.py --mixed --window 0.125 --check [--mixed-batch 512] [--mixed-orders 8,256] [--itype 1]
                                                 the variable window check (ek_hip_check_window_xvbatched_device;
                                                 --itype 2 / 3: ek_hip_check_sygv_window_xvbatched_device) on that
                                                 workload's m, w and Z: against a uniform window-check call per distinct
                                                 order, against the variable window solve that produced the pairs and
                                                 against the full variable check on the full solve of the same batch

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
    def __init__(self, lib, n, batch, distinct=64, itype=1):
        self.lib, self.n, self.batch, self.itype = lib, n, batch, itype
        A, B = pairs(n, min(batch, distinct), n)
        reps = -(-batch // A.shape[0])
        self.hA = np.ascontiguousarray(np.tile(A, (reps, 1, 1))[:batch]).ravel()
        self.hB = np.ascontiguousarray(np.tile(B, (reps, 1, 1))[:batch]).ravel()
        self.keep = []
        self.dA, self.dB, self.dZ = (self.alloc(batch * n * n * 8) for _ in range(3))
        self.dw = self.alloc(batch * n * 8)
        self.info = np.zeros(batch, dtype=np.int32)
        self.dA0 = self.dB0 = None                  # the original matrices, for the check (the solver works in place)

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
        fn, first = self.lib.ek_hip_eigenpairs_batched_device, problem
        if n > solver.XBATCH_NMAX:                  # orders 257 .. 512: the class of 512 rows
            fn = self.lib.ek_hip_eigenpairs_ybatched_device
            if problem and self.itype != 1:
                fn, first = self.lib.ek_hip_sygv_ybatched_device, self.itype
        elif n > solver.BATCH_NMAX:                 # orders 129 .. 256: the image in device memory
            fn = self.lib.ek_hip_eigenpairs_xbatched_device
            if problem and self.itype != 1:
                fn, first = self.lib.ek_hip_sygv_xbatched_device, self.itype
        elif problem and self.itype != 1:
            fn, first = self.lib.ek_hip_sygv_batched_device, self.itype
        rc = fn(first, jobz, n, self.batch, self.dA, n, nn, self.dB if problem else None, n, nn, self.dw,
                self.dZ if jobz else None, n, nn, self.info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                ctypes.byref(sec))
        t = time.perf_counter() - t0
        assert rc == 0 and not self.info.any(), (rc, self.info[self.info != 0][:4])
        return t, sec.value

    def window(self, problem, jobz, il=None, iu=None, vl=None, vu=None, itype=1):
        """ek_hip_eigenpairs_window_batched_device (above BATCH_NMAX: ek_hip_eigenpairs_window_xbatched_device) by index
        (il, iu) or by value (vl, vu): wall, device, m.  itype 2 / 3 (problem 1): ek_hip_sygv_window_batched_device /
        ek_hip_sygv_window_xbatched_device."""
        n, nn = self.n, self.n * self.n
        self.restore()
        sec = ctypes.c_double(0.0)
        m = np.zeros(self.batch, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        by_value = vl is not None
        t0 = time.perf_counter()
        x = "xbatched" if n > solver.BATCH_NMAX else "batched"
        fn, first = getattr(self.lib, "ek_hip_eigenpairs_window_%s_device" % x), problem
        if problem and itype != 1:
            fn, first = getattr(self.lib, "ek_hip_sygv_window_%s_device" % x), itype
        rc = fn(
            first, jobz, 1 if by_value else 0, n, self.batch, vl if by_value else 0.0, vu if by_value else 0.0,
            il or 0, iu or 0, self.dA, n, nn, self.dB if problem else None, n, nn, m.ctypes.data_as(ip), self.dw,
            self.dZ if jobz else None, n, n, nn, self.info.ctypes.data_as(ip), ctypes.byref(sec))
        t = time.perf_counter() - t0
        assert rc == 0 and not self.info.any(), (rc, self.info[self.info != 0][:4])
        return t, sec.value, m

    def check(self, problem):
        """The batched check on what the last batched(problem, 1) left in dw and dZ: wall time, device time, out."""
        n, nn = self.n, self.n * self.n
        if self.dA0 is None:
            self.dA0, self.dB0 = self.alloc(self.hA.nbytes), self.alloc(self.hB.nbytes)
            assert self.lib.ek_hip_memcpy_h2d(self.dA0, self.hA.ctypes.data, self.hA.nbytes) == 0
            assert self.lib.ek_hip_memcpy_h2d(self.dB0, self.hB.ctypes.data, self.hB.nbytes) == 0
        out = np.zeros((self.batch, 4))
        ipr = np.zeros((self.batch, n))
        dp = ctypes.POINTER(ctypes.c_double)
        sec = ctypes.c_double(0.0)
        t0 = time.perf_counter()
        fn, first = self.lib.ek_hip_check_batched_device, problem
        if n > solver.BATCH_NMAX:                   # orders 129 .. 256: the check of the xbatched solver
            fn = self.lib.ek_hip_check_xbatched_device
        if problem and self.itype != 1:             # types 2 and 3: the type's own check behind the type's own solve
            first = self.itype
            fn = (self.lib.ek_hip_check_sygv_xbatched_device if n > solver.BATCH_NMAX
                  else self.lib.ek_hip_check_sygv_batched_device)
        rc = fn(first, n, self.batch, self.dA0, n, nn, self.dB0 if problem else None, n, nn, self.dw, self.dZ, n, nn,
                self.info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out.ctypes.data_as(dp), ipr.ctypes.data_as(dp),
                ctypes.byref(sec))
        t = time.perf_counter() - t0
        assert rc == 0, rc
        return t, sec.value, out

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


def mixed(lib, batch, lo, hi, check=False):
    """Generalized with vectors, orders drawn i.i.d. uniformly from lo..hi (seeded).  Best of 3 after a warm-up, the kinds
    alternated, inputs restored outside the clock.  Wall times; for the variable call also the device time and the time of
    every class's launch (events on its stream).  check: the variable acceptance check (ek_hip_check_xvbatched_device, or
    ek_hip_check_vbatched_device up to order 128) of the variable solve's results against one uniform check call per
    distinct order and against the solve itself, on the same workload."""
    ip = ctypes.POINTER(ctypes.c_int)
    orders = np.random.default_rng(2048).integers(lo, hi + 1, batch)
    mats = {}
    for n in np.unique(orders):                     # eight distinct pairs per order, reused round robin
        mats[int(n)] = pairs(int(n), 8, int(n))
    seen = {}
    A, B = [], []
    for n in orders:
        k = seen.get(int(n), 0)
        seen[int(n)] = k + 1
        A.append(mats[int(n)][0][k % 8].T.ravel())  # column-major (symmetric: the same either way)
        B.append(mats[int(n)][1][k % 8].T.ravel())
    off = np.concatenate(([0], np.cumsum(orders.astype(np.int64) ** 2)))
    woff = np.concatenate(([0], np.cumsum(orders.astype(np.int64))))
    hA, hB = np.concatenate(A), np.concatenate(B)
    by_order = np.argsort(orders, kind="stable")
    gA, gB = np.concatenate([A[b] for b in by_order]), np.concatenate([B[b] for b in by_order])
    goff = np.concatenate(([0], np.cumsum(orders[by_order].astype(np.int64) ** 2)))
    gwoff = np.concatenate(([0], np.cumsum(orders[by_order].astype(np.int64))))
    distinct, first, counts = np.unique(orders[by_order], return_index=True, return_counts=True)
    big = hi > solver.BATCH_NMAX                    # the entries for orders up to 256
    pad = Case(lib, solver.XBATCH_NMAX if big else solver.BATCH_NMAX, batch)
    f_var = lib.ek_hip_eigenpairs_xvbatched_device if big else lib.ek_hip_eigenpairs_vbatched_device
    f_uni = lib.ek_hip_eigenpairs_xbatched_device if big else lib.ek_hip_eigenpairs_batched_device

    keep = []

    def up(a):
        p = ctypes.c_void_p()
        assert lib.ek_hip_malloc(ctypes.byref(p), int(a.nbytes)) == 0
        keep.append(p)
        return p

    def put(p, a):
        assert lib.ek_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0

    dA, dB, dgA, dgB = up(hA), up(hB), up(gA), up(gB)
    dw, dZ = pad.dw, pad.dZ                         # large enough for every kind
    n32 = orders.astype(np.int32)
    info = np.zeros(batch, dtype=np.int32)

    def table(base, offs):
        return (ctypes.c_void_p * batch)(*[base.value + int(offs[b]) * 8 for b in range(batch)])

    tA, tB, tw, tZ = table(dA, off), table(dB, off), table(dw, woff), table(dZ, off)

    def var():
        put(dA, hA); put(dB, hB)
        sec = ctypes.c_double(0.0)
        t0 = time.perf_counter()
        rc = f_var(1, 1, batch, n32.ctypes.data_as(ip), tA, n32.ctypes.data_as(ip), tB, n32.ctypes.data_as(ip), tw, tZ,
                   n32.ctypes.data_as(ip), info.ctypes.data_as(ip), ctypes.byref(sec))
        t = time.perf_counter() - t0
        assert rc == 0 and not info.any(), (rc, info[info != 0][:4])
        cls, cnt = np.zeros(4), np.zeros(4, dtype=np.int32)
        assert lib.ek_hip_debug_xvbatched_last(cls.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                               cnt.ctypes.data_as(ip)) == 0
        if not big:                                 # the three classes of ek_hip_eigenpairs_vbatched*
            assert cnt[0] == 0
            cls, cnt = cls[1:], cnt[1:]
        return t, sec.value, cls, cnt

    def grouped():
        put(dgA, gA); put(dgB, gB)
        t = 0.0
        at = lambda p, o: ctypes.c_void_p(p.value + int(o) * 8)  # noqa: E731
        for n, f, c in zip(distinct, first, counts):
            n, c = int(n), int(c)
            t0 = time.perf_counter()
            rc = f_uni(1, 1, n, c, at(dgA, goff[f]), n, n * n, at(dgB, goff[f]), n, n * n, at(dw, gwoff[f]),
                       at(dZ, goff[f]), n, n * n, info.ctypes.data_as(ip), None)
            t += time.perf_counter() - t0
            assert rc == 0 and not info[:c].any()
        return t

    if check:
        mixed_check(lib, batch, orders, by_order, (distinct, first, counts), (off, woff, goff, gwoff), (hA, hB, gA, gB),
                    (dA, dB, dgA, dgB, dw, dZ), (tw, tZ), var, up, put, table, big)
        for p in keep:
            lib.ek_hip_free(p)
        pad.close()
        return
    if big:
        print("# mixed: %d generalized problems with vectors, orders %d..%d (%d distinct; classes of 256 / 128 / 64 / 32: "
              "%d / %d / %d / %d)" % (batch, lo, hi, len(distinct), (orders > 128).sum(),
                                      ((orders > 64) & (orders <= 128)).sum(), ((orders > 32) & (orders <= 64)).sum(),
                                      (orders <= 32).sum()))
    else:
        print("# mixed: %d generalized problems with vectors, orders %d..%d (%d distinct; classes of 128 / 64 / 32: %d / %d / %d)"
              % (batch, lo, hi, len(distinct), (orders > 64).sum(), ((orders > 32) & (orders <= 64)).sum(),
                 (orders <= 32).sum()))
    res = {}
    for streams in (3, 1):
        assert lib.ek_hip_debug_vbatched_streams(streams) == 0
        tv, tg, tp = [], [], []
        var(); grouped(); pad.batched(1, 1)             # warm-up
        for _ in range(3):
            tv.append(var()); tg.append(grouped()); tp.append(pad.batched(1, 1)[0])
        best = min(tv, key=lambda x: x[0])
        res[streams] = best[0]
        names = ("256", "128", "64", "32")[-len(best[2]):]
        print("  streams=%d | t_var wall %.3f ms device %.3f ms | class launches %s | "
              "t_grouped %.3f ms (ratio %.1f) | t_pad %.3f ms (ratio %.2f)"
              % (streams, best[0] * 1e3, best[1] * 1e3,
                 "  ".join("%s: %.3f ms" % (k, v * 1e3) for k, v in zip(names, best[2])),
                 min(tg) * 1e3, min(tg) / best[0], min(tp) * 1e3, min(tp) / best[0]), flush=True)
        print("            all t_var wall ms: %s" % " ".join("%.3f" % (x[0] * 1e3) for x in tv))
    assert lib.ek_hip_debug_vbatched_streams(3) == 0
    for p in keep:
        lib.ek_hip_free(p)
    pad.close()


def mixed_check(lib, batch, orders, by_order, groups, offsets, host, device, tables, var, up, put, table, big):
    """--mixed --check: the rest of mixed() for the checks.  The solve runs once per round (its device time is the
    yardstick of the "no dearer than the solve" rule); its w and Z stay where the variable call left them and are copied
    once, ordered by order, for the uniform calls."""
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    distinct, first, counts = groups
    off, woff, goff, gwoff = offsets
    hA, hB, gA, gB = host
    dA, dB, dgA, dgB, dw, dZ = device
    tw, tZ = tables
    c_var = lib.ek_hip_check_xvbatched_device if big else lib.ek_hip_check_vbatched_device
    c_uni = lib.ek_hip_check_xbatched_device if big else lib.ek_hip_check_batched_device
    dA0, dB0 = up(hA), up(hB)                       # the originals, the variable call's layout
    put(dA0, hA); put(dB0, hB)
    tA0, tB0 = table(dA0, off), table(dB0, off)
    n32 = orders.astype(np.int32)
    info = np.zeros(batch, dtype=np.int32)
    out = np.zeros(batch * 4)
    q = np.zeros(int(woff[-1]))
    tq = (ctypes.c_void_p * batch)(*[q.ctypes.data + int(woff[b]) * 8 for b in range(batch)])
    gout, gq = np.zeros(batch * 4), np.zeros(int(gwoff[-1]))
    var()                                           # warm-up of the solve; its w and Z feed every check below
    hw, hZ = np.zeros(int(woff[-1])), np.zeros(int(off[-1]))
    assert lib.ek_hip_memcpy_d2h(hw.ctypes.data, dw, hw.nbytes) == 0
    assert lib.ek_hip_memcpy_d2h(hZ.ctypes.data, dZ, hZ.nbytes) == 0
    gw = np.concatenate([hw[woff[b]:woff[b + 1]] for b in by_order])
    gZ = np.concatenate([hZ[off[b]:off[b + 1]] for b in by_order])
    dgw, dgZ = up(gw), up(gZ)
    put(dgw, gw); put(dgZ, gZ)
    put(dgA, gA); put(dgB, gB)

    def check_var():
        sec = ctypes.c_double(0.0)
        t0 = time.perf_counter()
        rc = c_var(1, batch, n32.ctypes.data_as(ip), tA0, n32.ctypes.data_as(ip), tB0, n32.ctypes.data_as(ip), tw, tZ,
                   n32.ctypes.data_as(ip), info.ctypes.data_as(ip), out.ctypes.data_as(dp), tq, ctypes.byref(sec))
        t = time.perf_counter() - t0
        assert rc == 0, rc
        cls, cnt = np.zeros(4), np.zeros(4, dtype=np.int32)
        assert lib.ek_hip_debug_check_xvbatched_last(cls.ctypes.data_as(dp), cnt.ctypes.data_as(ip)) == 0
        return t, sec.value, cls, cnt

    def check_grouped():
        t = 0.0
        at = lambda p, o: ctypes.c_void_p(p.value + int(o) * 8)  # noqa: E731
        for n, f, c in zip(distinct, first, counts):
            n, f, c = int(n), int(f), int(c)
            t0 = time.perf_counter()
            rc = c_uni(1, n, c, at(dgA, goff[f]), n, n * n, at(dgB, goff[f]), n, n * n, at(dgw, gwoff[f]),
                       at(dgZ, goff[f]), n, n * n, None, gout[4 * f:].ctypes.data_as(dp), gq[gwoff[f]:].ctypes.data_as(dp),
                       None)
            t += time.perf_counter() - t0
            assert rc == 0, rc
        return t

    print("# mixed check: %d generalized problems, orders %d..%d (%d distinct; classes of 256 / 128 / 64 / 32: "
          "%d / %d / %d / %d), IPRs wanted, device-resident"
          % (batch, orders.min(), orders.max(), len(distinct), (orders > 128).sum(),
             ((orders > 64) & (orders <= 128)).sum(), ((orders > 32) & (orders <= 64)).sum(), (orders <= 32).sum()))
    check_var(); check_grouped()                    # warm-up
    tv, tg, ts = [], [], []
    for _ in range(3):
        ts.append(var()[1])                         # the same bits every time: the checks' inputs do not move
        tv.append(check_var()); tg.append(check_grouped())
    best = min(tv, key=lambda x: x[0])
    dev = min(x[1] for x in tv)
    o, g = out.reshape(batch, 4), gout.reshape(batch, 4)
    same = all(np.array_equal(o[b].view(np.uint64), g[k].view(np.uint64))
               and np.array_equal(q[woff[b]:woff[b + 1]].view(np.uint64), gq[gwoff[k]:gwoff[k + 1]].view(np.uint64))
               for k, b in enumerate(by_order))
    print("  t_var wall %.3f ms device %.3f ms | classes %s | t_grouped (%d calls) %.3f ms (ratio %.1f) | solve device "
          "%.3f ms (check / solve %.3f) | same bits both ways: %s | worst res_max %.2e orthogonality %.2e"
          % (best[0] * 1e3, dev * 1e3,
             "  ".join("%s: %d, %.3f ms" % (k, c, v * 1e3) for k, c, v in zip(("256", "128", "64", "32"), best[3], best[2])),
             len(distinct), min(tg) * 1e3, min(tg) / best[0], min(ts) * 1e3, dev / min(ts), same, o[:, 2].max(),
             o[:, 3].max()), flush=True)
    print("            all t_var wall ms: %s" % " ".join("%.3f" % (x[0] * 1e3) for x in tv))


def window_rows(lib, sizes, batches, fractions):
    """Device ms, best of 3, the kinds alternated: the existing call, and a window of each fraction of n by index and by
    value (bounds at the window's ends in the first problem's spectrum, so that the count varies over the batch)."""
    import scipy.linalg as sl
    print("# problem     n batch fraction | full jobz=1  jobz=0 | window 'I' jobz=1 (ratio)  'V' jobz=1 (ratio, mean m)  "
          "'I' jobz=0 (ratio to full jobz=0)")
    for n in sizes:
        for batch in batches:
            c = Case(lib, n, batch)
            A0 = c.hA[:n * n].reshape(n, n).T
            B0 = c.hB[:n * n].reshape(n, n).T
            for problem in (1, 0):
                w0 = sl.eigh(A0, B0, eigvals_only=True) if problem else sl.eigh(A0, eigvals_only=True)
                for f in fractions:
                    m = max(1, int(round(f * n)))
                    vl, vu = -np.inf, (0.5 * (w0[m - 1] + w0[m]) if m < n else np.inf)
                    kinds = {"f1": lambda: c.batched(problem, 1)[1], "f0": lambda: c.batched(problem, 0)[1],
                             "i1": lambda: c.window(problem, 1, il=1, iu=m)[1],
                             "v1": lambda: c.window(problem, 1, vl=vl, vu=vu)[1],
                             "i0": lambda: c.window(problem, 0, il=1, iu=m)[1]}
                    best = {}
                    for rep in range(4):            # the first round warms up
                        for k, fn in kinds.items():
                            t = fn()
                            if rep:
                                best[k] = min(best.get(k, np.inf), t)
                    mv = c.window(problem, 1, vl=vl, vu=vu)[2].mean()
                    print("  %7d %5d %5d %8.3f | %11.3f %7.3f | %17.3f (%.3f) %11.3f (%.3f, %.1f) %11.3f (%.3f)"
                          % (problem, n, batch, f, best["f1"] * 1e3, best["f0"] * 1e3, best["i1"] * 1e3,
                             best["i1"] / best["f1"], best["v1"] * 1e3, best["v1"] / best["f1"], mv, best["i0"] * 1e3,
                             best["i0"] / best["f0"]), flush=True)
            c.close()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import batched_cases as bc
    print("# fully clustered standard batches, every pair wanted: full jobz=1 ms | window 1..n jobz=1 ms (ratio)")
    for n in sizes:
        for name in ("all_equal", "two_clusters"):
            c = Case(lib, n, batches[0])
            c.hA = np.ascontiguousarray(np.tile(bc.make(name, n).A.T, (batches[0], 1, 1))).ravel()
            best = {}
            for rep in range(4):
                for k, fn in (("f1", lambda: c.batched(0, 1)[1]), ("i1", lambda: c.window(0, 1, il=1, iu=n)[1])):
                    t = fn()
                    if rep:
                        best[k] = min(best.get(k, np.inf), t)
            print("  %-14s n=%d batch=%d | %9.3f | %9.3f (%.3f)"
                  % (name, n, batches[0], best["f1"] * 1e3, best["i1"] * 1e3, best["i1"] / best["f1"]), flush=True)
            c.close()


def sygv_window_rows(lib, sizes, batches, fractions, itype):
    """Device ms, best of 3, the kinds alternated: the window call of type itype (2 / 3) by index against the full call of
    the same type (ek_hip_sygv_batched_device / ek_hip_sygv_xbatched_device) and against the type-1 window call."""
    print("# itype %d     n batch fraction | full jobz=1  jobz=0 | window 'I' jobz=1 (of full, of type 1's window)  "
          "'I' jobz=0 (of full jobz=0, of type 1's)" % itype)
    for n in sizes:
        for batch in batches:
            c = Case(lib, n, batch, itype=itype)
            for f in fractions:
                m = max(1, int(round(f * n)))
                kinds = {"f1": lambda: c.batched(1, 1)[1], "f0": lambda: c.batched(1, 0)[1],
                         "i1": lambda: c.window(1, 1, il=1, iu=m, itype=itype)[1],
                         "i0": lambda: c.window(1, 0, il=1, iu=m, itype=itype)[1],
                         "t1": lambda: c.window(1, 1, il=1, iu=m)[1], "t0": lambda: c.window(1, 0, il=1, iu=m)[1]}
                best = {}
                for rep in range(4):                # the first round warms up
                    for k, fn in kinds.items():
                        t = fn()
                        if rep:
                            best[k] = min(best.get(k, np.inf), t)
                print("  %7d %5d %5d %8.3f | %11.3f %7.3f | %17.3f (%.3f, %.3f) %21.3f (%.3f, %.3f)"
                      % (itype, n, batch, f, best["f1"] * 1e3, best["f0"] * 1e3, best["i1"] * 1e3,
                         best["i1"] / best["f1"], best["i1"] / best["t1"], best["i0"] * 1e3, best["i0"] / best["f0"],
                         best["i0"] / best["t0"]), flush=True)
            c.close()


def mixed_window(lib, batch, lo, hi, fraction, itype):
    """The variable-order window call against its three alternatives (module docstring): generalized problems of orders
    drawn uniformly from lo .. hi, the lowest max(1, fraction n) pairs with vectors.  One warm-up of each kind, then three
    rounds that alternate the kinds, best device time; the inputs are restored outside the clock."""
    I = ctypes.POINTER(ctypes.c_int)
    D = ctypes.POINTER(ctypes.c_double)
    rng = np.random.default_rng(2024)
    orders = np.sort(rng.integers(lo, hi + 1, size=batch))         # the problems of an order stand behind each other
    distinct = np.unique(orders)
    N = int(orders.max())
    seeds = {int(n): pairs(500 + int(n), 1, int(n)) for n in distinct}
    offm = np.concatenate([[0], np.cumsum(orders.astype(np.int64) ** 2)])
    offw = np.concatenate([[0], np.cumsum(orders.astype(np.int64))])
    hA, hB = np.empty(offm[-1]), np.empty(offm[-1])
    PA, PB = np.zeros((batch, N, N)), np.zeros((batch, N, N))
    PA[:, np.arange(N), np.arange(N)] = 1e6                         # the padding's eigenvalues lie above every window
    PB[:, np.arange(N), np.arange(N)] = 1.0
    for b, n in enumerate(orders):
        A, B = seeds[int(n)]
        hA[offm[b]:offm[b + 1]], hB[offm[b]:offm[b + 1]] = A[0].ravel(), B[0].ravel()
        PA[b, :n, :n], PB[b, :n, :n] = A[0], B[0]
    PA, PB = PA.ravel(), PB.ravel()
    keep = []

    def alloc(nbytes):
        p = ctypes.c_void_p()
        assert lib.ek_hip_malloc(ctypes.byref(p), int(max(nbytes, 8))) == 0
        keep.append(p)
        return p

    def put(p, a):
        assert lib.ek_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0

    dA, dB, dZ, dw = alloc(hA.nbytes), alloc(hB.nbytes), alloc(hA.nbytes), alloc(offw[-1] * 8)
    dPA, dPB, dPZ, dPw = alloc(PA.nbytes), alloc(PB.nbytes), alloc(PA.nbytes), alloc(batch * N * 8)
    perm = rng.permutation(batch)

    def table(base, off):
        return (ctypes.c_void_p * batch)(*[base.value + int(off[b]) * 8 for b in perm])

    def at(p, off):
        return ctypes.c_void_p(p.value + int(off) * 8)

    tA, tB, tw, tZ = table(dA, offm), table(dB, offm), table(dw, offw), table(dZ, offm)
    n32 = orders[perm].astype(np.int32)
    il = np.ones(batch, dtype=np.int32)
    iu = np.maximum(1, (fraction * n32).astype(np.int32)).astype(np.int32)
    m, info = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    sec = np.zeros(1)
    ip = lambda a: a.ctypes.data_as(I)              # noqa: E731
    first = itype if itype != 1 else 1
    wentry = lib.ek_hip_sygv_window_xvbatched_device if itype != 1 else lib.ek_hip_eigenpairs_window_xvbatched_device
    fentry = lib.ek_hip_sygv_xvbatched_device if itype != 1 else lib.ek_hip_eigenpairs_xvbatched_device
    uentry = lib.ek_hip_sygv_window_xbatched_device if itype != 1 else lib.ek_hip_eigenpairs_window_xbatched_device

    def variable():
        put(dA, hA); put(dB, hB)
        rc = wentry(first, 1, 0, batch, ip(n32), None, None, ip(il), ip(iu), tA, ip(n32), tB, ip(n32), ip(m), tw, tZ,
                    ip(n32), ip(iu), ip(info), sec.ctypes.data_as(D))
        assert rc == 0 and not info.any() and (m == iu).all(), (rc, info[info != 0][:4])
        return float(sec[0])

    def full():
        put(dA, hA); put(dB, hB)
        rc = fentry(first, 1, batch, ip(n32), tA, ip(n32), tB, ip(n32), tw, tZ, ip(n32), ip(info), sec.ctypes.data_as(D))
        assert rc == 0 and not info.any()
        return float(sec[0])

    def per_order():
        put(dA, hA); put(dB, hB)
        t = 0.0
        for n in distinct:
            n = int(n)
            f, c, k = int(np.searchsorted(orders, n)), int((orders == n).sum()), max(1, int(fraction * n))
            rc = uentry(first, 1, 0, n, c, 0.0, 0.0, 1, k, at(dA, offm[f]), n, n * n, at(dB, offm[f]), n, n * n, ip(m),
                        at(dw, offw[f]), at(dZ, offm[f]), n, k, n * n, ip(info), sec.ctypes.data_as(D))
            assert rc == 0 and not info[:c].any()
            t += float(sec[0])
        return t

    kmax = max(1, int(fraction * N))

    def padded():
        put(dPA, PA); put(dPB, PB)
        rc = uentry(first, 1, 0, N, batch, 0.0, 0.0, 1, kmax, dPA, N, N * N, dPB, N, N * N, ip(m), dPw, dPZ, N, kmax,
                    N * N, ip(info), sec.ctypes.data_as(D))
        assert rc == 0 and not info.any()
        return float(sec[0])

    print("# %d generalized problems (itype %d) of orders %d..%d (%d distinct), the lowest max(1, %g n) pairs with vectors"
          % (batch, itype, lo, hi, len(distinct), fraction))
    for streams in (3, 1):
        lib.ek_hip_debug_vbatched_streams(streams)
        tv, tf, tg, tp = [], [], [], []
        variable(); full(); per_order(); padded()      # warm-up
        for _ in range(3):
            tv.append(variable()); tf.append(full()); tg.append(per_order()); tp.append(padded())
        variable()
        csec, ccnt = np.zeros(4), np.zeros(4, dtype=np.int32)
        lib.ek_hip_debug_xvbatched_last(csec.ctypes.data_as(D), ip(ccnt))
        print("  streams %d: variable window %.3f ms | full variable call %.3f ms (window / full %.3f) | window call per "
              "order %.3f ms (%.1f x) | padded to %d: %.3f ms (%.2f x)"
              % (streams, min(tv) * 1e3, min(tf) * 1e3, min(tv) / min(tf), min(tg) * 1e3, min(tg) / min(tv), N,
                 min(tp) * 1e3, min(tp) / min(tv)))
        print("             classes 256 / 128 / 64 / 32: %s ms, %s problems"
              % (" / ".join("%.3f" % (x * 1e3) for x in csec), " / ".join(str(x) for x in ccnt)), flush=True)
    lib.ek_hip_debug_vbatched_streams(3)
    for p in keep:
        lib.ek_hip_free(p)


def mixed_window_check(lib, batch, lo, hi, fraction, itype):
    """The variable window check (ek_hip_check_window_xvbatched_device; --itype 2 / 3:
    ek_hip_check_sygv_window_xvbatched_device) on the workload of mixed_window: against a uniform window-check call per
    distinct order, against the variable window solve that produced the pairs, and against the full variable check on
    the full solve of the same batch.  One warm-up of each kind, then three rounds that alternate the kinds; device
    seconds (the checks do not touch their inputs), and the wall clock of the two ways to check the windows."""
    I = ctypes.POINTER(ctypes.c_int)
    D = ctypes.POINTER(ctypes.c_double)
    rng = np.random.default_rng(2024)
    orders = np.sort(rng.integers(lo, hi + 1, size=batch)).astype(np.int64)
    distinct = np.unique(orders)
    cols = np.maximum(1, (fraction * orders).astype(np.int64))
    seeds = {int(n): pairs(500 + int(n), 1, int(n)) for n in distinct}
    offm = np.concatenate([[0], np.cumsum(orders ** 2)])
    offw = np.concatenate([[0], np.cumsum(orders)])
    offz = np.concatenate([[0], np.cumsum(orders * cols)])
    hA, hB = np.empty(offm[-1]), np.empty(offm[-1])
    for b, n in enumerate(orders):
        A, B = seeds[int(n)]
        hA[offm[b]:offm[b + 1]], hB[offm[b]:offm[b + 1]] = A[0].ravel(), B[0].ravel()
    keep = []

    def alloc(nbytes):
        p = ctypes.c_void_p()
        assert lib.ek_hip_malloc(ctypes.byref(p), int(max(nbytes, 8))) == 0
        keep.append(p)
        return p

    def put(p, a):
        assert lib.ek_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0

    dA0, dB0, dA, dB = (alloc(hA.nbytes) for _ in range(4))
    dw, dZ, dwf, dZf = alloc(offw[-1] * 8), alloc(offz[-1] * 8), alloc(offw[-1] * 8), alloc(hA.nbytes)
    put(dA0, hA); put(dB0, hB)
    perm = rng.permutation(batch)

    def table(base, off):
        return (ctypes.c_void_p * batch)(*[base.value + int(off[b]) * 8 for b in perm])

    def at(p, off):
        return ctypes.c_void_p(p.value + int(off) * 8)

    tA0, tB0, tA, tB = table(dA0, offm), table(dB0, offm), table(dA, offm), table(dB, offm)
    tw, tZ, twf, tZf = table(dw, offw), table(dZ, offz), table(dwf, offw), table(dZf, offm)
    n32 = orders[perm].astype(np.int32)
    il = np.ones(batch, dtype=np.int32)
    iu = cols[perm].astype(np.int32)
    m, info = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    mu = np.zeros(batch, dtype=np.int32)
    out = np.zeros((batch, 4))
    sec = np.zeros(1)
    ip = lambda a: a.ctypes.data_as(I)              # noqa: E731
    dp = lambda a: a.ctypes.data_as(D)              # noqa: E731
    if itype != 1:
        wsolve, fsolve = lib.ek_hip_sygv_window_xvbatched_device, lib.ek_hip_sygv_xvbatched_device
        vcheck, ucheck = lib.ek_hip_check_sygv_window_xvbatched_device, lib.ek_hip_check_sygv_window_xbatched_device
        fcheck = lib.ek_hip_check_sygv_xvbatched_device
    else:
        wsolve, fsolve = lib.ek_hip_eigenpairs_window_xvbatched_device, lib.ek_hip_eigenpairs_xvbatched_device
        vcheck, ucheck = lib.ek_hip_check_window_xvbatched_device, lib.ek_hip_check_window_xbatched_device
        fcheck = lib.ek_hip_check_xvbatched_device

    def solve():
        put(dA, hA); put(dB, hB)
        rc = wsolve(itype, 1, 0, batch, ip(n32), None, None, ip(il), ip(iu), tA, ip(n32), tB, ip(n32), ip(m), tw, tZ,
                    ip(n32), ip(iu), ip(info), dp(sec))
        assert rc == 0 and not info.any() and (m == iu).all(), (rc, info[info != 0][:4])
        return float(sec[0])

    def variable():
        t0 = time.perf_counter()
        rc = vcheck(itype, batch, ip(n32), tA0, ip(n32), tB0, ip(n32), ip(m), tw, tZ, ip(n32), ip(iu), ip(info), dp(out),
                    None, dp(sec))
        assert rc == 0
        return float(sec[0]), time.perf_counter() - t0

    def per_order():
        t, t0 = 0.0, time.perf_counter()
        for n in distinct:
            n = int(n)
            f, c, k = int(np.searchsorted(orders, n)), int((orders == n).sum()), max(1, int(fraction * n))
            mu[:c] = k
            rc = ucheck(itype, n, c, at(dA0, offm[f]), n, n * n, at(dB0, offm[f]), n, n * n, ip(mu), at(dw, offw[f]),
                        at(dZ, offz[f]), n, k, n * k, None, dp(out), None, dp(sec))
            assert rc == 0
            t += float(sec[0])
        return t, time.perf_counter() - t0

    def full():
        rc = fcheck(itype, batch, ip(n32), tA0, ip(n32), tB0, ip(n32), twf, tZf, ip(n32), ip(info), dp(out), None, dp(sec))
        assert rc == 0
        return float(sec[0])

    put(dA, hA); put(dB, hB)
    rc = fsolve(itype, 1, batch, ip(n32), tA, ip(n32), tB, ip(n32), twf, tZf, ip(n32), ip(info), None)
    assert rc == 0 and not info.any()
    solve()                                         # warm-up of each kind
    ts = [solve() for _ in range(3)]
    variable(); per_order(); full()
    tv, tvw, tu, tuw, tf = [], [], [], [], []
    for _ in range(3):
        a, b = variable()
        worst = (float(out[:, 2].max()), float(out[:, 3].max()))
        c, d = per_order()
        tv.append(a); tvw.append(b); tu.append(c); tuw.append(d); tf.append(full())
    print("# check of %d generalized problems (itype %d) of orders %d..%d (%d distinct), the lowest max(1, %g n) pairs"
          % (batch, itype, lo, hi, len(distinct), fraction))
    print("  variable window check %.3f ms (wall %.3f ms) | uniform window check per order %.3f ms (%.1f x; wall %.3f ms, "
          "%.1f x) | variable window solve %.3f ms (check / solve %.4f) | full variable check of the full solve %.3f ms "
          "(window / full %.3f) | worst res_max %.2e, orthogonality %.2e"
          % (min(tv) * 1e3, min(tvw) * 1e3, min(tu) * 1e3, min(tu) / min(tv), min(tuw) * 1e3, min(tuw) / min(tvw),
             min(ts) * 1e3, min(tv) / min(ts), min(tf) * 1e3, min(tv) / min(tf), worst[0], worst[1]), flush=True)
    for p in keep:
        lib.ek_hip_free(p)


def window_check_rows(lib, sizes, batches, fractions, loop_max, itype=1):
    """The window of max(1, fraction n) pairs from index n / 4 + 1, with vectors.  Per (problem, n, batch, fraction): a
    warm-up, then three rounds of window solve, window check, full check (on a full solve's w and Z, made once) and the
    host loop over ek_hip_check_sygvx_device (min(batch, loop_max) problems, scaled; the standard problem gets B = I);
    device times, wall for the loop and beside the window check.  itype 2 / 3: the generalized rows alone, with
    ek_hip_check_sygv_window_xbatched_device behind the type's window solve, the type's full check and the type's loop."""
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    print("# %s     n batch     m | window solve ms | window check wall ms  device ms | full check ms | loop ms (scaled) | "
          "window / full  window / solve  loop / window | worst res_max  orthogonality"
          % ("problem" if itype == 1 else "  itype"))
    for n in sizes:
        nn = n * n
        for batch in batches:
            c = Case(lib, n, batch, itype=itype)
            win = (c.dw, c.dZ)
            full = (c.alloc(batch * n * 8), c.alloc(batch * nn * 8))
            dI = c.alloc(nn * 8)
            eye = np.eye(n).ravel()
            assert lib.ek_hip_memcpy_h2d(dI, eye.ctypes.data, eye.nbytes) == 0
            out, ipr = np.zeros((batch, 4)), np.zeros((batch, n))
            one, q1 = np.zeros(4), np.zeros(n)
            count = min(batch, loop_max)
            at = lambda p, b, per: ctypes.c_void_p(p.value + b * per * 8)  # noqa: E731
            wcheck, first = lib.ek_hip_check_window_xbatched_device, None
            if itype != 1:
                wcheck, first = lib.ek_hip_check_sygv_window_xbatched_device, itype
            for problem in ((1, 0) if itype == 1 else (1,)):
                c.dw, c.dZ = full
                c.batched(problem, 1)
                c.check(problem)                    # makes the kept originals dA0, dB0
                c.dw, c.dZ = win
                for f in fractions:
                    mcols = max(1, int(f * n))
                    il = min(n // 4 + 1, n - mcols + 1)
                    iu = il + mcols - 1
                    ts, tw, tf, tl, worst = [], [], [], [], np.zeros(2)
                    for rep in range(4):            # the first round warms up
                        _, d, m = c.window(problem, 1, il=il, iu=iu, itype=itype)
                        ts.append(d)
                        sec = ctypes.c_double(0.0)
                        t0 = time.perf_counter()
                        rc = wcheck(
                            problem if first is None else first, n, batch, c.dA0, n, nn, c.dB0 if problem else None, n, nn, m.ctypes.data_as(ip), c.dw,
                            c.dZ, n, n, nn, c.info.ctypes.data_as(ip), out.ctypes.data_as(dp), ipr.ctypes.data_as(dp),
                            ctypes.byref(sec))
                        tw.append((sec.value, time.perf_counter() - t0))
                        assert rc == 0 and np.all(m == mcols), (rc, m[:4])
                        worst = np.maximum(worst, [out[:, 2].max(), out[:, 3].max()])
                        c.dw, c.dZ = full
                        tf.append(c.check(problem)[1])
                        c.dw, c.dZ = win
                        t0 = time.perf_counter()
                        for b in range(count):
                            rc = lib.ek_hip_check_sygvx_device(itype, n, mcols, at(c.dA0, b, nn), n,
                                                               at(c.dB0, b, nn) if problem else dI, n, at(c.dw, b, n),
                                                               at(c.dZ, b, nn), n, one.ctypes.data_as(dp),
                                                               q1.ctypes.data_as(dp))
                            assert rc == 0, rc
                        tl.append((time.perf_counter() - t0) * (batch / count))
                    d, t = min(tw[1:])
                    s, fc, lo = min(ts[1:]), min(tf[1:]), min(tl[1:])
                    print("  %7d %5d %5d %5d | %15.3f | %20.3f %10.3f | %13.3f | %16.2f | %13.3f %15.3f %14.1f | %13.2e %14.2e"
                          % (problem if itype == 1 else itype, n, batch, mcols, s * 1e3, t * 1e3, d * 1e3, fc * 1e3, lo * 1e3, d / fc, d / s, lo / t,
                             worst[0], worst[1]), flush=True)
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30,64,128")
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--loop-max", type=int, default=64)
    ap.add_argument("--itype", type=int, choices=(1, 2, 3), default=1,
                    help="problem type of the generalized batched rows (2, 3: ek_hip_sygv_batched_device, "
                         "ek_hip_sygv_xbatched_device above order 128)")
    ap.add_argument("--once", default=None, help="<n>g or <n>s: one generalized / standard batch of 256 with vectors")
    ap.add_argument("--once-batch", type=int, default=256)
    ap.add_argument("--check", action="store_true", help="time the batched check behind each solve (with vectors); with "
                    "--mixed: the variable check against a uniform check call per distinct order and against its solve")
    ap.add_argument("--mixed", action="store_true", help="problems of different orders: the variable call "
                    "(an upper order above 128: ek_hip_eigenpairs_xvbatched_device)")
    ap.add_argument("--mixed-batch", type=int, default=2048)
    ap.add_argument("--mixed-orders", default="8,128", help="lo,hi of the uniformly drawn orders")
    ap.add_argument("--window", default=None, help="fractions of n, e.g. 0.125,1: the window call by index and by value "
                    "against the existing call, then fully clustered batches")
    args = ap.parse_args()
    lib = solver.load_library()
    assert lib.ek_hip_init(0) == 0
    if args.mixed and args.window:
        lo, hi = (int(x) for x in args.mixed_orders.split(","))
        for fraction in (float(x) for x in args.window.split(",")):
            (mixed_window_check if args.check else mixed_window)(lib, args.mixed_batch, lo, hi, fraction, args.itype)
        lib.ek_hip_finalize()
        return
    if args.window and args.itype != 1 and not args.check:
        sygv_window_rows(lib, [int(x) for x in args.sizes.split(",")], [int(x) for x in args.batches.split(",")],
                         [float(x) for x in args.window.split(",")], args.itype)
        lib.ek_hip_finalize()
        return
    if args.window and args.check:
        window_check_rows(lib, [int(x) for x in args.sizes.split(",")], [int(x) for x in args.batches.split(",")],
                          [float(x) for x in args.window.split(",")], args.loop_max, args.itype)
        lib.ek_hip_finalize()
        return
    if args.window:
        window_rows(lib, [int(x) for x in args.sizes.split(",")], [int(x) for x in args.batches.split(",")],
                    [float(x) for x in args.window.split(",")])
        lib.ek_hip_finalize()
        return
    if args.mixed:
        lo, hi = (int(x) for x in args.mixed_orders.split(","))
        mixed(lib, args.mixed_batch, lo, hi, check=args.check)
        lib.ek_hip_finalize()
        return
    if args.once:
        n, problem = int(args.once[:-1]), 1 if args.once.endswith("g") else 0
        c = Case(lib, n, args.once_batch, itype=args.itype)
        c.batched(problem, 1)
        if args.check:
            c.check(problem)
        t, dev = c.batched(problem, 1)
        print("once: n=%d problem=%d batch=%d wall %.3f ms device %.3f ms"
              % (n, problem, args.once_batch, t * 1e3, dev * 1e3))
        if args.check:
            t, dev, out = c.check(problem)
            print("once: the check on its w and Z: wall %.3f ms device %.3f ms, worst res_max %.2e orthogonality %.2e"
                  % (t * 1e3, dev * 1e3, out[:, 2].max(), out[:, 3].max()))
        c.close()
        lib.ek_hip_finalize()
        return
    if args.check:
        if args.itype != 1:
            print("# generalized rows: itype %d (ek_hip_check_sygv_batched_device behind ek_hip_sygv_batched_device; "
                  "ek_hip_check_sygv_xbatched_device behind ek_hip_sygv_xbatched_device above order %d)"
                  % (args.itype, solver.BATCH_NMAX))
        print("# problem     n batch | solve device ms | check wall ms  device ms  us/problem | check / solve | "
              "worst res_max  orthogonality")
        for n in (int(x) for x in args.sizes.split(",")):
            for batch in (int(x) for x in args.batches.split(",")):
                c = Case(lib, n, batch, itype=args.itype)
                for problem in (1, 0):
                    ts, tc, worst = [], [], np.zeros(2)
                    c.batched(problem, 1); c.check(problem)                         # warm-up
                    for _ in range(3):
                        ts.append(c.batched(problem, 1)[1])
                        t, d, out = c.check(problem)
                        tc.append((d, t))
                        worst = np.maximum(worst, [out[:, 2].max(), out[:, 3].max()])
                    d, t = min(tc)
                    print("  %7d %5d %5d | %15.3f | %13.3f %10.3f %11.2f | %13.3f | %13.2e %14.2e"
                          % (problem, n, batch, min(ts) * 1e3, t * 1e3, d * 1e3, d / batch * 1e6, d / min(ts), worst[0],
                             worst[1]), flush=True)
                c.close()
        lib.ek_hip_finalize()
        return
    if args.itype != 1:
        print("# generalized rows: itype %d (ek_hip_sygv_batched_device; ek_hip_sygv_xbatched_device above order %d)"
              % (args.itype, solver.BATCH_NMAX))
    print("# problem jobz     n batch | batched wall ms  device ms  us/problem  problems/s | loop ms (scaled)  "
          "us/problem | ratio")
    for n in (int(x) for x in args.sizes.split(",")):
        for batch in (int(x) for x in args.batches.split(",")):
            c = Case(lib, n, batch, itype=args.itype)
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
