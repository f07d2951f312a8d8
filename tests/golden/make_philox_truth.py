"""Writes tests/golden/philox_truth.npz: the 50-digit truth of the normal stream (tests/philox_truth.py) on a bulk block and
at the extremes of the transform.  Run from the repository root:  python tests/golden/make_philox_truth.py [out.npz]
(about two minutes: a vectorised host search over 2^28 pairs of counters, then mpmath on ~15 500 pairs).

Bulk: rows 0..15 x BULK_COLS columns for each of BULK_TRIPLES.
Extremes, found by the search over rows 0..3 (each the lower row of a pair) x columns 0 .. 2^26 - 1 at (SEARCH_SEED,
SEARCH_STEP) -- columns below 2^31, so that one pls_normal_fill of 8 x 1 with j_offset = column fetches a pair:
  the 16 smallest u1, the 16 u1 closest to 1, per octant the 4 smallest and the 4 largest positions t, and the 16 pairs with the
  smallest |z| on either row (64 candidates by the numpy formula, ranked by mpmath).  Both rows of every pair are kept."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import philox_truth as T  # noqa: E402

SEARCH_COLS_LOG2, CHUNK_LOG2 = 26, 21


def keep_smallest(pool, keys, payload, n):
    """merge (keys, payload rows) into ``pool`` and keep the n smallest keys (ties: the smaller counters, deterministic)"""
    if pool is not None:
        keys, payload = np.concatenate([pool[0], keys]), np.concatenate([pool[1], payload])
    order = np.lexsort((payload[:, 1], payload[:, 0], keys))[:n]
    return keys[order], payload[order]


def search():
    """-> {regime index: (n, 2) array of (ibase, column)}"""
    pools = {}
    rows = np.arange(4, dtype=np.uint64)[:, None]
    p50 = np.uint64((1 << 50) - 1)
    for c0 in range(0, 1 << SEARCH_COLS_LOG2, 1 << CHUNK_LOG2):
        cols = np.arange(c0, c0 + (1 << CHUNK_LOG2), dtype=np.uint64)[None, :]
        a, b = T.uniforms53(*T.words(rows, cols, T.SEARCH_STEP, T.SEARCH_SEED))
        ncols = 1 << CHUNK_LOG2
        a, b = a.ravel(), b.ravel()
        o, p = T.octant_position(b)

        def offer(regime, keys, n, mask=None):
            idx = np.flatnonzero(mask) if mask is not None else np.arange(keys.size)
            k = keys[idx]
            if k.size > 4 * n:
                part = np.argpartition(k, 4 * n)[: 4 * n]
                idx, k = idx[part], k[part]
            ctr = np.stack([idx // ncols, c0 + idx % ncols], axis=1).astype(np.uint64)  # (ibase, column)
            pools[regime] = keep_smallest(pools.get(regime), k.astype(np.float64), ctr, n)

        offer(T.R_SMALL_U1, a, 16)
        offer(T.R_U1_ONE, np.uint64((1 << 53) - 1) - a, 16)
        for oc in range(8):
            offer(T.R_OCT_LOW + oc, p, 4, o == oc)
            offer(T.R_OCT_HIGH + oc, p50 - p, 4, o == oc)
        u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -53
        u2 = (b.astype(np.float64) + 0.5) * 2.0 ** -53
        rad = np.sqrt(-2.0 * np.log(u1))
        offer(T.R_SMALL_Z, rad * np.minimum(np.abs(np.cos(2 * np.pi * u2)), np.abs(np.sin(2 * np.pi * u2))), 64)
        print(f"searched columns below {c0 + (1 << CHUNK_LOG2)}", flush=True)
    # the small |z| candidates ranked by the truth itself
    cand = pools[T.R_SMALL_Z][1]
    a, b = T.uniforms53(*T.words(cand[:, 0], cand[:, 1], T.SEARCH_STEP, T.SEARCH_SEED))
    best = np.array([min(abs(h) for h, _ in T.pair_truth(x, y)) for x, y in zip(a, b)])
    pools[T.R_SMALL_Z] = keep_smallest(None, best, cand, 16)
    return {r: v[1] for r, v in pools.items()}


def main(out_path):
    out = {"bulk_triples": np.array(T.BULK_TRIPLES, dtype=np.uint64)}
    nb = len(T.BULK_TRIPLES)
    hi = np.empty((nb, T.BULK_ROWS, T.BULK_COLS))
    lo = np.empty_like(hi)
    wd = np.empty((nb, T.BULK_ROWS // 2, T.BULK_COLS, 4), dtype=np.uint32)
    ibases = np.array([i for i in range(T.BULK_ROWS) if not i & 4], dtype=np.uint64)
    for t, (seed, step, joff) in enumerate(T.BULK_TRIPLES):
        jg = (np.arange(T.BULK_COLS, dtype=np.uint64) + np.uint64(joff)) & np.uint64(0xFFFFFFFF)
        x = T.words(ibases[:, None], jg[None, :], step, seed)
        wd[t] = np.stack(x, axis=-1).astype(np.uint32)
        a, b = T.uniforms53(*x)
        for k, ib in enumerate(ibases.tolist()):
            for c in range(T.BULK_COLS):
                (h0, l0), (h1, l1) = T.pair_truth(a[k, c], b[k, c])
                hi[t, ib, c], lo[t, ib, c], hi[t, ib + 4, c], lo[t, ib + 4, c] = h0, l0, h1, l1
        print(f"bulk block {t} done", flush=True)
    out.update(bulk_hi=hi, bulk_lo=lo, bulk_words=wd)

    found = search()
    rows, cols, regime, ehi, elo, ewd = [], [], [], [], [], []
    for r in sorted(found):
        for ib, col in found[r].tolist():
            x = T.words(ib, col, T.SEARCH_STEP, T.SEARCH_SEED)
            a, b = T.uniforms53(*x)
            for h, (vh, vl) in enumerate(T.pair_truth(a, b)):
                rows.append(ib + 4 * h)
                cols.append(col)
                regime.append(r)
                ehi.append(vh)
                elo.append(vl)
                ewd.append([int(w) for w in x])
    out.update(ext_row=np.array(rows, dtype=np.int64), ext_col=np.array(cols, dtype=np.int64),
               ext_step=np.full(len(rows), T.SEARCH_STEP, dtype=np.uint64), ext_seed=np.full(len(rows), T.SEARCH_SEED, dtype=np.uint64),
               ext_regime=np.array(regime, dtype=np.int8), ext_hi=np.array(ehi), ext_lo=np.array(elo),
               ext_words=np.array(ewd, dtype=np.uint32), search_pairs_log2=np.array(SEARCH_COLS_LOG2 + 2))
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes, {nb * T.BULK_ROWS * T.BULK_COLS // 2 + len(rows) // 2} pairs")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE)
