"""Pure-Python restatement of NumPy 1.x ``argsort(kind="quicksort")``: the scalar introsort ``aquicksort_`` with its
``aheapsort_`` fallback (numpy/core/src/npysort/quicksort.cpp, heapsort.cpp).  NumPy before 1.25 runs it on every CPU; later
NumPy runs it when SIMD sort dispatch is disabled.  pandas ``sort_values(by=col)`` (``nargsort``, kind="quicksort") on a column
without NaNs is this permutation.  Every comparison is a strict ``<`` on the keys.

``argsort(keys, stats)`` also records in ``stats["heapsort"]`` how many ranges fell back to the heapsort."""
from __future__ import annotations

SMALL_QUICKSORT = 15                # a range of 16 or fewer elements is insertion-sorted


def _msb(n):
    depth = 0
    while n > 1:
        n >>= 1
        depth += 1
    return depth


def _aheapsort(k, a, lo, n):
    """aheapsort_ on a[lo .. lo+n-1], written on a 1-based view as NumPy does"""
    def at(i):
        return a[lo + i - 1]

    def put(i, v):
        a[lo + i - 1] = v

    def sift(tmp, i, n):
        j = 2 * i
        while j <= n:
            if j < n and k[at(j)] < k[at(j + 1)]:
                j += 1
            if k[tmp] < k[at(j)]:
                put(i, at(j))
                i = j
                j += j
            else:
                break
        put(i, tmp)

    for l in range(n >> 1, 0, -1):
        sift(at(l), l, n)
    while n > 1:
        tmp = at(n)
        put(n, at(1))
        n -= 1
        sift(tmp, 1, n)


def argsort(keys, stats=None):
    k = keys.tolist() if hasattr(keys, "tolist") else list(keys)       # anything with a strict <
    n = len(k)
    a = list(range(n))
    if stats is not None:
        stats.setdefault("heapsort", 0)
    if n == 0:
        return a
    pl, pr = 0, n - 1
    cdepth = _msb(n) * 2
    stack, depths = [], []
    while True:
        if cdepth < 0:
            _aheapsort(k, a, pl, pr - pl + 1)
            if stats is not None:
                stats["heapsort"] += 1
        else:
            while pr - pl > SMALL_QUICKSORT:
                pm = pl + ((pr - pl) >> 1)
                if k[a[pm]] < k[a[pl]]:
                    a[pm], a[pl] = a[pl], a[pm]
                if k[a[pr]] < k[a[pm]]:
                    a[pr], a[pm] = a[pm], a[pr]
                if k[a[pm]] < k[a[pl]]:
                    a[pm], a[pl] = a[pl], a[pm]
                vp = k[a[pm]]
                pi, pj = pl, pr - 1
                a[pm], a[pj] = a[pj], a[pm]
                while True:
                    pi += 1
                    while k[a[pi]] < vp:
                        pi += 1
                    pj -= 1
                    while vp < k[a[pj]]:
                        pj -= 1
                    if pi >= pj:
                        break
                    a[pi], a[pj] = a[pj], a[pi]
                a[pi], a[pr - 1] = a[pr - 1], a[pi]
                if pi - pl < pr - pi:
                    stack.append((pi + 1, pr))
                    pr = pi - 1
                else:
                    stack.append((pl, pi - 1))
                    pl = pi + 1
                cdepth -= 1
                depths.append(cdepth)
            for pi in range(pl + 1, pr + 1):                       # insertion sort, strict < : stable
                vi = a[pi]
                vp = k[vi]
                pj = pi
                while pj > pl and vp < k[a[pj - 1]]:
                    a[pj] = a[pj - 1]
                    pj -= 1
                a[pj] = vi
        if not stack:
            return a
        pl, pr = stack.pop()
        cdepth = depths.pop()
