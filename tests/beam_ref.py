"""The numpy-float32 reference of the beam stage (zig_gpt2_amd/csrc/sample_beam.h; include/zgpt2.h zg_beam_options): one beam
step over given top-2W lists with the state carried from column to column, and the host's finalisation with backtracking.

Every number the device compares or stores is float32 here too: the candidate's value is ONE float32 add, the normalised score ONE
float32 division by lenpow[L] = float32(pow(float64(L), float64(length_penalty))).  Orders are decided by comparisons alone:
value descending, then slot ascending, then list entry ascending; NaN below every number; -0.0 equal to +0.0.

THE TIE RULE of the pool: the worst entry is the one of lowest norm and, among equal norms, the one at the highest pool index; a
full pool takes an offer only if its norm is strictly greater than the worst entry's, in that entry's place."""
import math

import numpy as np

NO_EOS = None
F32 = np.float32


def lenpow(n, length_penalty):
    """lenpow[L], L = 0 .. n - 1 (entry 0 is never read: NaN here)."""
    out = np.full(n, np.nan, F32)
    for L in range(1, n):
        out[L] = F32(math.pow(float(L), float(F32(length_penalty))))
    return out


def _isnan(v):
    return bool(v != v)


def _order(v):
    """Sort key of a value under "descending, NaN last": smaller sorts first."""
    return (1, 0.0) if _isnan(v) else (0, -float(v))


def _gt(a, b):
    """a strictly greater than b, NaN below every number."""
    if _isnan(a):
        return False
    if _isnan(b):
        return True
    return bool(a > b)


def _worst(pool):
    """Index of the pool's worst entry (THE TIE RULE)."""
    w = 0
    for k in range(1, len(pool)):
        if not _gt(pool[k]["norm"], pool[w]["norm"]):  # lower or equal: the later index is the worse
            w = k
    return w


def offer(pool, W, entry):
    if len(pool) < W:
        pool.append(entry)
        return
    w = _worst(pool)
    if _gt(entry["norm"], pool[w]["norm"]):
        pool[w] = entry


class Beams:
    """The state of one beam generation over `batch` rows: G = batch // W groups of W slots."""

    def __init__(self, batch, W, eos=NO_EOS, length_penalty=1.0, early_stopping=True, c0=0, n_lenpow=4097):
        assert 1 <= W <= 8 and batch % W == 0
        self.B, self.W, self.G = batch, W, batch // W
        self.eos, self.early, self.c0 = eos, bool(early_stopping), c0
        self.length_penalty = float(F32(length_penalty))
        self.lenpow = lenpow(n_lenpow, length_penalty)
        self.score = np.array([0.0 if s % W == 0 else -np.inf for s in range(batch)], F32)
        self.pools = [[] for _ in range(self.G)]
        self.done_col = [-1] * self.G
        self.ranked = [[] for _ in range(self.G)]  # the kept candidates of each group's last step, in rank order: (value, slot, j, token)

    def step(self, ids, lps, col):
        """One beam step at column `col` over ids / lps [batch][2W] (lists by the slot BEFORE the step).  Returns (tokens, parents,
        scores, logprobs) [batch], by the slot AFTER the step."""
        B, W = self.B, self.W
        ids = np.asarray(ids).reshape(B, 2 * W)
        lps = np.asarray(lps, F32).reshape(B, 2 * W)
        tokens, parents = np.zeros(B, np.int32), np.zeros(B, np.int32)
        scores, logprobs = np.zeros(B, F32), np.zeros(B, F32)
        lp = self.lenpow[col - self.c0 + 1]
        for g in range(self.G):
            s0 = g * W
            if self.done_col[g] >= 0:  # identity parents, the slot's own top-1 token, the score as it stands
                for s in range(s0, s0 + W):
                    tokens[s], parents[s], scores[s], logprobs[s] = ids[s, 0], s, self.score[s], lps[s, 0]
                continue
            cands = []
            for sl in range(W):
                if col > self.c0 or sl == 0:
                    for j in range(2 * W):
                        cands.append((F32(self.score[s0 + sl] + lps[s0 + sl, j]), sl, j))  # float32 + float32: one rounded add
            cands.sort(key=lambda c: (_order(c[0]), c[1], c[2]))
            self.ranked[g] = [(v, s0 + sl, j, int(ids[s0 + sl, j])) for v, sl, j in cands[: 2 * W]]  # (for tests that choose an eos)
            beams = []
            for r, (v, sl, j) in enumerate(cands[: 2 * W]):
                tok = int(ids[s0 + sl, j])
                if self.eos is not None and tok == self.eos:
                    if r < W:
                        offer(self.pools[g], W, {"sum": v, "norm": F32(v / lp), "parent": s0 + sl, "col": col})
                    continue
                if len(beams) < W:
                    beams.append((v, sl, j, tok))
            pool = self.pools[g]
            if len(pool) >= W:
                worst = pool[_worst(pool)]["norm"]
                best = beams[0][0] if beams else F32(-np.inf)
                if self.early or bool(worst >= F32(best / lp)):
                    self.done_col[g] = col
            slot, taken = [None] * len(beams), set()
            for i, (_, sl, _, _) in enumerate(beams):
                if sl not in taken:
                    slot[i] = sl
                    taken.add(sl)
            for i in range(len(beams)):
                if slot[i] is None:
                    slot[i] = min(t for t in range(W) if t not in taken)
                    taken.add(slot[i])
            new_score = self.score.copy()
            for i, (v, sl, j, tok) in enumerate(beams):
                t = s0 + slot[i]
                tokens[t], parents[t], scores[t], logprobs[t] = tok, s0 + sl, v, lps[s0 + sl, j]
                new_score[t] = v
            for tl in range(W):
                if tl not in taken:  # no beam was found for the slot: it keeps itself, score -inf
                    t = s0 + tl
                    tokens[t], parents[t], scores[t], logprobs[t] = ids[t, 0], t, -np.inf, lps[t, 0]
                    new_score[t] = -np.inf
            self.score = new_score
        return tokens, parents, scores, logprobs

    def host_done_col(self):
        """The pinned word the kernel stores: the highest done column + 1 once every group is done, else 0."""
        return max(self.done_col) + 1 if all(d >= 0 for d in self.done_col) else 0

    def finalize(self, end, out_tokens, parents, n_return):
        """What zg_gpt_generate_fetch_beams returns: per group a list of (tokens, norm, sum) of the n_return best hypotheses.
        out_tokens / parents are indexed [row][column] by absolute column."""
        W, c0 = self.W, self.c0
        res = []
        for g in range(self.G):
            pool = [dict(e, eos=True) for e in self.pools[g]]
            if self.done_col[g] < 0:
                lp = F32(math.pow(float(end - c0), self.length_penalty))
                for s in range(g * W, g * W + W):
                    offer(pool, W, {"sum": self.score[s], "norm": F32(self.score[s] / lp), "parent": s, "col": end, "eos": False})
            order = sorted(range(len(pool)), key=lambda k: (_order(pool[k]["norm"]), k))
            hyps = []
            for k in order[:n_return]:
                e = pool[k]
                seq, cur = ([self.eos] if e["eos"] else []), e["parent"]
                for c in range(e["col"] - 1, c0 - 1, -1):
                    seq.append(int(out_tokens[cur][c]))
                    cur = int(parents[cur][c])
                hyps.append((seq[::-1], e["norm"], e["sum"]))
            res.append(hyps)
        return res


def bits(x):
    """float32 array -> its bit patterns, for bit-for-bit comparisons (NaN payloads included)."""
    return np.ascontiguousarray(x, F32).view(np.uint32)


# ---- lists for the tests of the stage
def random_lists(rng, W, V, eos, p_eos, ties, rows=None):
    """Lists for `rows` slots (default W: one group) of 2W entries each: distinct tokens within a slot, eos sprinkled in, values
    descending; ties: values on a coarse grid, so that sums are equal across slots and entries."""
    rows = W if rows is None else rows
    ids = np.stack([rng.permutation(V)[: 2 * W] for _ in range(rows)]).astype(np.int32)
    if eos is not None:
        for s in range(rows):
            if rng.random() < p_eos and eos not in ids[s]:
                ids[s, rng.integers(0, 2 * W)] = eos
    lps = -np.sort(rng.gamma(2.0, 1.0, (rows, 2 * W)).astype(np.float32), axis=1)
    if ties:
        lps = (np.round(lps * 2) / 2).astype(np.float32)
    return ids, np.sort(lps, axis=1)[:, ::-1].copy()


def lists(W, rows):
    """rows: per slot a list of (token, logprob) — padded to 2W entries with distinct filler tokens at -50."""
    ids = np.zeros((W, 2 * W), np.int32)
    lps = np.full((W, 2 * W), -50.0, np.float32)
    for s, row in enumerate(rows):
        for j in range(2 * W):
            ids[s, j], lps[s, j] = row[j] if j < len(row) else (900 + 10 * s + j, -50.0 - j)
    return ids, lps
