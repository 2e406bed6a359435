"""A host-side reference model of a GalleryIndex (not a test module).

The model holds what an index IS -- the gallery values as the index's dtype rounds them, the set of deleted rows, and
whether a row was ever deleted -- and nothing an index CACHES (norm bound, split, packed live words, per-lane masks and
workspaces).  Every mutation mirrors the index method of the same name on that state; every query is answered from the
state of the moment by the brute-force fp64 references the rest of the suite already trusts (search_helpers,
sweep_helpers, decide_helpers, assign_helpers, trim_helpers, oracle/search_ref.c).  An index whose caches went stale
differs from the model, and from ``fresh(index)``: a new index built from the same gallery with the same rows deleted.

``run`` names the fields of a method's complete return, ``same`` compares two such returns bit for bit and
``against_model`` compares one with what the model defines.  No comparison here has a tolerance.
"""
import numpy as np
import torch

import trim_helpers
from assign_helpers import oracle_assign
from decide_helpers import oracle_decide, unpack_words
from search_helpers import expect_topk, oracle_join, oracle_range
from sweep_helpers import oracle_sweep

MUTATIONS = ("none", "delete_rows", "update_rows", "restore_rows", "write_refresh", "dedup")


def seen(x, dtype) -> np.ndarray:
    """The fp32 values an index of ``dtype`` sees of ``x`` (tensor or array): rounded to the dtype once, widened back"""
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x.detach().cpu())
    return np.ascontiguousarray(t.to(dtype).to(torch.float32).numpy())


def _rows(rows) -> np.ndarray:
    if isinstance(rows, torch.Tensor):
        rows = rows.detach().cpu().numpy()
    return np.asarray(rows, dtype=np.int64).reshape(-1)


def _bool(m):
    if m is None:
        return None
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    return np.asarray(m, dtype=bool)


def query_masks(row_masks, N: int):
    """bool [Q, N] of a ``row_masks=`` argument: a bool tensor / array, or DecisionMasks (their words unpacked)"""
    if row_masks is None:
        return None
    if hasattr(row_masks, "words"):
        return unpack_words(row_masks.words.detach().cpu().numpy(), N)
    return _bool(row_masks)


class IndexModel:
    def __init__(self, gallery, dtype=None, presplit=None):
        """gallery: tensor [N, E] in the index's dtype (or anything, with ``dtype`` given)"""
        self.dtype = gallery.dtype if dtype is None else dtype
        self.g = seen(gallery, self.dtype).copy()
        self.N, self.E = self.g.shape
        self.dead = np.zeros(self.N, dtype=bool)
        self.ever_deleted = False
        self.presplit = presplit
        self._gmax = None

    # ------------------------------------------------------------------ mutations
    def update_rows(self, rows, values) -> None:
        """``gallery[rows] = values`` (duplicate ids: the last write wins, as one indexed assignment on the host does);
        a deleted row stays deleted"""
        self.g[_rows(rows)] = seen(values, self.dtype)
        self._gmax = None

    def write_refresh(self, rows, values) -> None:
        """A direct write into ``index.gallery`` followed by ``refresh_norm_bound()``: the same state as update_rows"""
        self.update_rows(rows, values)

    def delete_rows(self, rows) -> None:
        self.dead[_rows(rows)] = True
        self.ever_deleted = True

    def restore_rows(self, rows) -> None:
        self.dead[_rows(rows)] = False
        self.ever_deleted = True          # GalleryIndex creates its live buffers on the first _set_live, whichever way

    def dedup(self, ref, threshold, prefilter=None):
        """-> (dropped int64, partner int64): keep_first over the model's own join of the live rows, then their deletion"""
        from mmr_amd import dedup as _dedup

        i, j, _ = self.near_duplicates(ref, threshold, prefilter=prefilter)
        keep, dup = _dedup.keep_first(self.N, i, j)
        dropped = np.flatnonzero(~keep).astype(np.int64)
        if dropped.size:
            self.delete_rows(dropped)
        return dropped, dup[dropped].astype(np.int64)

    # ------------------------------------------------------------------ state
    @property
    def live(self) -> np.ndarray:
        return ~self.dead

    def mask(self, row_mask=None) -> np.ndarray:
        """live & row_mask"""
        m = _bool(row_mask)
        return self.live if m is None else self.live & m

    def _qmasks(self, Q, row_mask, row_masks):
        """bool [Q, N]: the AND of the live rows, the call's row_mask and each query's own mask"""
        base = self.mask(row_mask)
        qm = query_masks(row_masks, self.N)
        return np.broadcast_to(base, (Q, self.N)) if qm is None else qm & base[None, :]

    def max_norm(self) -> float:
        """the largest row norm (fp64 sums), kept until the next write"""
        if self._gmax is None:
            g = self.g.astype(np.float64)
            self._gmax = float(np.sqrt(np.einsum("ij,ij->i", g, g).max())) if self.N else 0.0
        return self._gmax

    def _slack(self, q) -> float:
        """search_helpers' window, scaled as its docstring says: 1e-6 |q| G"""
        qn = float(np.sqrt((np.asarray(q, dtype=np.float64) ** 2).sum(-1)).max()) if np.size(q) else 1.0
        return 1e-6 * max(qn * self.max_norm(), 1e-30)

    def fresh(self, index):
        """A new index over a copy of ``index``'s gallery, same ``presplit``, the model's dead rows deleted"""
        from mmr_amd.search import GalleryIndex

        f = GalleryIndex(index.gallery.clone(), norm_bound=index.norm_bound, presplit=index._presplit)
        if self.dead.any():
            f.delete_rows(np.flatnonzero(self.dead))
        return f

    # ------------------------------------------------------------------ queries
    def search(self, oracle, q, k, scale=1.0, row_mask=None, row_masks=None) -> dict:
        """search / search_deep (any k).  q: what the caller passes; seen in the index's dtype here"""
        q = seen(q, self.dtype)
        squeezed = q.ndim == 1
        q2 = q[None, :] if squeezed else q
        if row_masks is None:
            idx, score, d64 = expect_topk(oracle, torch.from_numpy(q2), torch.from_numpy(self.g), self.mask(row_mask), k, scale)
        else:
            qm = self._qmasks(q2.shape[0], row_mask, row_masks)
            parts = [expect_topk(oracle, torch.from_numpy(q2[a:a + 1]), torch.from_numpy(self.g), qm[a], k, scale)
                     for a in range(q2.shape[0])]
            idx, score, d64 = (np.concatenate([p[i] for p in parts]) for i in range(3))
        if squeezed:
            idx, score, d64 = idx[0], score[0], d64[0]
        return {"idx": idx.astype(np.int64), "score": score, "dot64": d64}

    def search_packed(self, oracle, q, k, scale, row_offset, row_mask=None) -> dict:
        r = self.search(oracle, q, k, scale, row_mask)
        ids = np.where(r["idx"] >= 0, r["idx"] + int(row_offset), -1)
        return {"packed": np.stack([ids, r["dot64"].view(np.int64)], axis=-1)}

    def range_search(self, ref, q, tau, scale=1.0, row_mask=None) -> dict:
        q = seen(q, self.dtype)
        qs, rs, d = oracle_range(ref, q, self.g, tau, self.mask(row_mask), slack=self._slack(q))
        offsets = np.concatenate([[0], np.cumsum(np.bincount(qs, minlength=q.shape[0]))]).astype(np.int64)
        return {"offsets": offsets, "idx": rs.astype(np.int64), "dot64": d,
                "score": (d * np.float64(np.float32(scale))).astype(np.float32)}

    def near_duplicates(self, ref, tau, row_mask=None, prefilter=None):
        """-> (i, j, dot64).  oracle_join over the rows that can be in a pair: ``prefilter(mask)`` (default: every masked
        row) names them, a superset found with a window far wider than its own arithmetic's error; the exact decision
        and the bits are oracle_join's"""
        mask = self.mask(row_mask)
        rows = np.flatnonzero(mask) if prefilter is None else np.sort(prefilter(self, tau, mask))
        if rows.size == 0:
            e = np.empty(0, dtype=np.int64)
            return e, e, np.empty(0, dtype=np.float64)
        sub = np.ascontiguousarray(self.g[rows])
        a, b, d = oracle_join(ref, sub, tau, slack=1e-6 * max(self.max_norm() ** 2, 1e-30))
        return rows[a], rows[b], d

    def threshold_sweep(self, ref, q, labels, targets, thresholds, row_mask=None, row_masks=None) -> dict:
        q = seen(q, self.dtype)
        labels, targets = np.asarray(labels), np.asarray(targets)
        if row_masks is None:
            ge, total, _ = oracle_sweep(ref, q, self.g, labels, targets, thresholds, self.mask(row_mask))
        else:
            qm = self._qmasks(q.shape[0], row_mask, row_masks)
            # query a over the compacted gallery g[qm[a]]: the same counts, without a pass over the rows it leaves out
            parts = []
            for a in range(q.shape[0]):
                rows = np.flatnonzero(qm[a])
                parts.append(oracle_sweep(ref, q[a:a + 1], np.ascontiguousarray(self.g[rows]), labels[rows], targets[a:a + 1], thresholds))
            ge, total = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        return {"tp": ge[:, 1], "fp": ge[:, 0], "pos": total[:, 1], "neg": total[:, 0]}

    def decide(self, ref, q, thr, row_mask=None) -> dict:
        q = seen(q, self.dtype)
        if q.ndim == 1:
            q = q[None, :]
        thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), (q.shape[0],))
        return {"words": oracle_decide(ref, q, self.g, thr, self.mask(row_mask), slack=self._slack(q))}

    def assign(self, ref, centroids, bias=None, row_mask=None) -> dict:
        c = seen(centroids, self.dtype)
        b = None if bias is None else np.asarray(bias.detach().cpu().numpy() if isinstance(bias, torch.Tensor) else bias, dtype=np.float64)
        labels, best, _ = oracle_assign(ref, self.g, c, b, self.mask(row_mask))
        return {"labels": labels, "best64": best}

    def trimmed_centers(self, labels, K, centers64, metric="cosine", percentile=95.0, row_mask=None) -> dict:
        """trim_helpers.restate with the labels of the masked rows set to -1.  The centres of the kept rows are a device
        sum in an order of its own: the model defines the rows kept, not that sum"""
        lab = np.where(self.mask(row_mask), np.asarray(labels), -1).astype(np.int32)
        r = trim_helpers.restate(self.g, lab, K, np.asarray(centers64, dtype=np.float64), metric, qs=(percentile,))
        return {"keep": r.trimmed[percentile] >= 0, "thresholds": r.thresholds[percentile], "kept": r.kept[percentile],
                "sizes": (r.start[1:] - r.start[:-1]).astype(np.int64)}

    def scores(self, oracle, ref_feature, scale=100.0) -> dict:
        r = seen(ref_feature, self.dtype)
        s = oracle.similarity(r, self.g, scale)                  # [Q, N]
        return {"scores": s[0] if r.ndim == 1 else np.ascontiguousarray(s.T)}

    def score_extent(self, oracle, q, row_mask=None) -> dict:
        """Two k = 1 oracle searches: of q, and of -q (negating a query negates every fixed-order dot exactly)"""
        q = seen(q, self.dtype)
        hi = self.search(oracle, q, 1, 1.0, row_mask)["dot64"][..., 0]
        lo = -self.search(oracle, -q, 1, 1.0, row_mask)["dot64"][..., 0]
        return {"lo": lo, "hi": hi}


def pair_rows(model: IndexModel, tau: float, mask: np.ndarray) -> np.ndarray:
    """The masked rows that have a partner with fp32 product >= tau - 1e-3 G^2 (blocked torch fp32 products; their error
    is below E 2^-24 G^2 < 5e-5 G^2 for E <= 768): a superset of the rows of every pair near or above ``tau``, so that
    oracle_join need not form the [N, N] fp64 matrix of a 20011-row gallery at every step"""
    rows = np.flatnonzero(mask)
    g = torch.from_numpy(model.g[rows])
    window = 1e-3 * model.max_norm() ** 2
    hit = np.zeros(rows.size, dtype=bool)
    for s in range(0, rows.size, 2048):
        p = g[s:s + 2048] @ g.T
        n = p.shape[0]
        p[torch.arange(n), torch.arange(s, s + n)] = -float("inf")
        hit[s:s + n] = (p >= tau - window).any(1).numpy()
    return rows[hit]


# ------------------------------------------------------------------ the fixtures of the margin-follows-the-state tests
CROWD_TAU = 0.5
CROWD_GRID = np.array([0.3, 0.5, 0.7])
CROWD_Q, CROWD_E, CROWD_N = 8, 128, 20010          # + the appended zero row: 20011 rows
# the long row's norm in units of G0.  4 for fp16.  Rounding a row to bf16 moves its dot by about 1.7e-4 (one sigma, E = 128),
# two margins eps(G0) = 8e-5, so the bf16 crowd is wider than the tau +- 3 eps(G0) it was drawn from: the window
# 0.9 eps(4 G0) = 3.6 eps(G0) holds 79 % of it, 0.9 eps(8 G0) holds 99.1 %
CROWD_LONG = {torch.bfloat16: 8.0, torch.float16: 4.0}
# the seed: with it no pair outside a query's own crowd lies within 0.9 eps(G1) of ANY grid point, for either dtype (seed 0
# leaves one bf16 outsider near 0.3); test_index_model_host.py asserts it
CROWD_SEED = 2


class LifecycleCrowd:
    """margin_helpers.crowd_fixture (unit rows, each query's own rows spread over tau +- 3 eps(G0)) plus one all-zero row
    at the end, and ``long`` = CROWD_LONG[dtype] w in the dtype, w a unit vector orthogonal to every query: written into
    the last row it makes the largest norm G1 = 4 G0 (8 G0 for bf16), widens every margin as much and matches nothing."""

    def __init__(self, dtype, seed=CROWD_SEED):
        import margin_helpers as M

        self.dtype = dtype
        q, g, dots = M.crowd_fixture(dtype, CROWD_E, CROWD_N, CROWD_Q, CROWD_TAU, seed)
        self.q = q
        self.g = torch.cat([g, torch.zeros(1, CROWD_E, dtype=dtype)]).contiguous()
        self.row = CROWD_N
        gen = torch.Generator().manual_seed(4100 + seed)
        w = torch.randn(CROWD_E, generator=gen, dtype=torch.float64)
        basis, _ = torch.linalg.qr(q.double().t())                   # [E, Q] orthonormal span of the queries
        w = w - basis @ (basis.t() @ w)
        self.factor = CROWD_LONG[dtype]
        self.long = (self.factor * w / w.norm()).to(dtype)
        self.qf = M.f32(q)
        self.own = (np.arange(CROWD_N) % CROWD_Q)[None, :] == np.arange(CROWD_Q)[:, None]        # [Q, CROWD_N]
        self.dots = dots                                             # [Q, CROWD_N]: the crowd rows
        self.long_dots = self.qf.astype(np.float64) @ M.f32(self.long).astype(np.float64)
        self.G0 = M.max_norm(M.f32(g))
        self.G1 = M.max_norm(M.f32(self.long)[None, :])
        self.eps0 = M.doc_margin("plain", self.qf, self.G0)[:, None]
        self.eps1 = M.doc_margin("plain", self.qf, self.G1)[:, None]
        near = np.abs(self.dots[:, :, None] - CROWD_GRID[None, None, :]).min(-1)
        self.near = {"decide": np.abs(self.dots - CROWD_TAU), "sweep": near}      # distance to the nearest threshold

    def floor(self, what: str) -> int:
        """pairs within 0.9 eps(G1) of a threshold: what counts[1] must reach once the long row is in"""
        return int((self.near[what] <= 0.9 * self.eps1).sum())

    def narrow(self, what: str) -> int:
        """pairs within 1.5 eps(G0): an upper estimate of what a scan still on the stale bound lists"""
        return int((self.near[what] <= 1.5 * self.eps0).sum())


class LifecycleAligned:
    """margin_helpers.aligned_gallery_fixture(128) with every row rounded to bf16 -- which turns the planted and anti rows
    into gh and leaves the decoys as they are -- as the gallery an index is BUILT over (``before``: its residual bound is
    exactly 0), and the rows ``update_rows`` then writes: planted = gh + DELTA s, anti = gh - DELTA s (``after``)."""

    def __init__(self, E=128):
        import margin_helpers as M

        fx = M.aligned_gallery_fixture(E)
        self.fx = fx
        self.before = M.bf16_round(fx.g)
        self.after = self.before.copy()
        self.after[fx.planted] = fx.g[fx.planted]
        self.after[fx.anti] = fx.g[fx.anti]
        self.q = fx.q


# ------------------------------------------------------------------ the complete return of a method, field by field
def _names(method, kw):
    if method == "search":
        return ["score", "idx"] + (["dot64"] if kw.get("return_dot64") else []) + (["status"] if kw.get("return_status") else [])
    if method == "search_deep":
        return ["score", "idx"] + (["dot64"] if kw.get("return_dot64") else [])
    if method == "range_search":
        return ["offsets", "idx", "score"] + (["dot64"] if kw.get("return_dot64") else [])
    return {"search_packed": ["packed"], "near_duplicates": ["i", "j", "score", "dot64"], "score_extent": ["lo", "hi"],
            "scores": ["scores"], "dedup": ["dropped", "partner"],
            "assign": ["labels", "best64"] if kw.get("return_score") else ["labels"]}[method]


def run(index, method, *args, **kw) -> dict:
    """``index.method(*args, **kw)`` as a dict of named fields: every tensor it returns, ``status``, the ``counts`` of a
    DecisionMasks / ThresholdSweep, and ``deep_counts`` after a search_deep"""
    ret = getattr(index, method)(*args, **kw)
    if method == "decide":
        return {"words": ret.words, "num_rows": ret.num_rows, "counts": tuple(ret.counts)}
    if method == "threshold_sweep":
        return {"tp": ret.tp, "fp": ret.fp, "pos": ret.pos, "neg": ret.neg, "thresholds": ret.thresholds, "counts": tuple(ret.counts)}
    if method == "trimmed_centers":
        return dict(ret._asdict())
    if not isinstance(ret, tuple):
        ret = (ret,)
    names = _names(method, kw)
    if method == "search" and kw.get("row_masks") is not None:
        names = [n for n in names if n != "status"]
    assert len(names) == len(ret), (method, names, len(ret))
    out = dict(zip(names, ret))
    if method == "search_deep" or (method == "search" and kw.get("row_masks") is not None):
        out["deep_counts"] = tuple(index.deep_counts)
    return out


def _bits(x):
    """(dtype, shape, raw bytes) of a tensor or array; other values as they are"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def same(a: dict, b: dict):
    """Two complete returns (``run``) bit for bit -> the name of the first field that differs, or None"""
    if list(a) != list(b):
        return "fields"
    for name in a:
        if _bits(a[name]) != _bits(b[name]):
            return name
    return None


def _canon(x):
    """numpy, integer ids as int64, words as uint32, every NaN as the one quiet NaN (a NaN's payload is not a value)"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    x = np.ascontiguousarray(x)
    if x.dtype.kind == "f":
        x = x.copy()
        x[np.isnan(x)] = np.nan
        return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])
    if x.dtype.kind in "iu" and x.dtype.itemsize == 4:
        return x.view(np.uint32).astype(np.int64)
    return x


def against_model(got: dict, want: dict):
    """A return (``run``) against the model's fields, exactly -> the name of the first model field the return lacks or
    differs in, or None.  Fields the model does not define (fp32 scores of pair lists aside, counts, status) are not
    looked at here: ``same`` against the fresh index covers them"""
    for name, w in want.items():
        if name not in got:
            return name
        g, w = _canon(got[name]), _canon(w)
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g, w):
            return name
    return None
