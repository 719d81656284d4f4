"""Score regimes of the stage tests' attention cases: how a case's `regime` field changes its weights and its tokens, the float64
forward that shows what the change does to the scores, and a float32 emulation of a split attention kernel that the teeth
tests of test_decode_stage_cases_cpu.py / test_pass_stage_cases_cpu.py break in four ways.  numpy only.

A model with N(0, 0.02) weights everywhere has near-uniform attention: LayerNorm normalises c_attn's input, so q and k have the
standard deviation 0.02 sqrt(E) and a scaled score 4e-4 E: +-0.05 at E = 128.  A trained checkpoint's scores spread over tens of
units, one key often takes nearly all of the mass, and whole key ranges underflow.  The regimes (all on one-layer models, where
q and k are a LayerNorm and a Linear away from the embedding, so that the conditions below hold by construction and are
asserted from a float64 forward on the CPU):

trained      rows [0, 2E) of c_attn_w times a power of two (q rows 2^ceil(g / 2), k rows 2^floor(g / 2): bf16 values stay bf16
             values), g from the width and the key count so that the spread max - min of every head's scores lies in [8, 60].
one-key@P    head 0 looks for position P whatever the query: wpe[P] is a row of the size of TOK_MEAN's (std 2), which the
             LayerNorm turns into a direction u; head 0's k rows are s_d sigma (u / 4 + sqrt(15 / 16) n_d) with fresh standard normal n_d
             — 64 weak detectors of u, so that no single k output is a sum of like-signed products — times ONE_KEY_K_GAIN, and
             head 0's q bias is ONE_KEY_Q_BIAS s_d: the score of key j is a constant times u . a_j, largest by far at P.  Position P
             holds 1 - 2^-24 of the mass or more for every query that sees it.
far-below    head 0's k rows and k bias are minus its q rows and q bias, q rows times 32 and k rows times 16, and every position
             of a sequence is fed one token (TOK_MEAN or TOK_OUT: rows that dwarf wpe): every score of head 0 is about -|q|^2 / 8,
             below -104 = ln 2^-150, so a running maximum started at 0 underflows every term, denormals included."""
import numpy as np

import stage_ref as sr

REGIMES = ("trained", "one-key", "far-below")
SPREAD = (8.0, 60.0)        # trained: every head's float64 score spread over the keys it sees
ONE_KEY_MASS = 2.0 ** -24   # one-key: what the other keys hold together, at the most
FAR_BELOW = -104.0          # far-below: every score of head 0 (ln 2^-149 = -103.3: the smallest float32 denormal)
Y_FLOOR = 2.0 ** -25        # trained: the float32 yardstick has not collapsed — an output of the size of its s is off by up to 2^-24 of
#                             it from its final rounding alone, and over hundreds of outputs the worst is above half of that unless
#                             the softmax has degenerated to one key (where it measures 1e-12)
ONE_KEY_K_GAIN, ONE_KEY_Q_BIAS, ONE_KEY_RHO = 16.0, 2.0, 0.25
FAR_BELOW_GAINS = (32.0, 16.0)


def parse(regime):
    """"" -> (None, None); "trained" / "far-below" -> (name, None); "one-key@255" -> ("one-key", 255)."""
    if not regime:
        return None, None
    name, _, hot = regime.partition("@")
    assert name in REGIMES and (name == "one-key") == bool(hot), regime
    return name, int(hot) if hot else None


def trained_power(E, keys):
    """g of the trained regime: the scores of a head at gain 1 are about N(0, (4e-4 E)^2), the range of `keys` of them about
    2 sqrt(2 ln keys) standard deviations (2.5 at the least); 2^g brings that to 36, or what the rounding of g
    makes of it: 25 .. 51, inside [8, 60] with room for the heads' own variation.  Below 32 keys the aim is 22: a handful of
    keys 36 apart leaves all of the mass on one of them, which is the one-key regime's business."""
    rng_sd = max(2.0 * np.sqrt(2.0 * np.log(max(keys, 2))), 2.5)
    return int(round(np.log2((36.0 if keys >= 32 else 22.0) / (4e-4 * E * rng_sd))))


def apply(w, regime, E, keys, seed):
    """The regime's change of a one-layer weight set w (in place; bf16-representable values stay so)."""
    name, hot = parse(regime)
    if name is None:
        return w
    bf = sr.round_bf16
    W, b = w["h0.c_attn_w"], w["h0.c_attn_b"]
    q0, k0 = slice(0, 64), slice(E, E + 64)  # head 0's q and k rows
    if name == "trained":
        g = trained_power(E, keys)
        W[:E] *= np.float32(2.0 ** ((g + 1) // 2))
        W[E:2 * E] *= np.float32(2.0 ** (g // 2))
    elif name == "far-below":
        W[q0] *= np.float32(FAR_BELOW_GAINS[0])
        W[k0] = -W[q0] * np.float32(FAR_BELOW_GAINS[1] / FAR_BELOW_GAINS[0])
        b[k0] = -b[q0]
    else:
        rng = np.random.default_rng(seed)
        row = bf(rng.standard_normal(E, dtype=np.float32) * np.float32(2.0))
        w["wpe"][hot] = row
        u = (row - row.mean()) / row.std()
        sign = np.where(rng.random(64) < 0.5, -1.0, 1.0).astype(np.float32)
        det = ONE_KEY_RHO * u[None, :] + np.sqrt(1.0 - ONE_KEY_RHO ** 2) * rng.standard_normal((64, E))
        W[k0] = bf((ONE_KEY_K_GAIN * 0.02 * sign[:, None] * det).astype(np.float32))
        b[q0] = bf(b[q0] + np.float32(ONE_KEY_Q_BIAS) * sign)
    return w


def same_token_rows(name, tokens, tok_even, tok_odd):
    """far-below feeds every position of sequence b one token: tok_even / tok_odd by b.  tokens: any [B][...] integer array."""
    if name == "far-below":
        tokens = tokens.copy()
        for b in range(tokens.shape[0]):
            tokens[b] = tok_even if b % 2 == 0 else tok_odd
    return tokens


# ---------------------------------------------------------------------------------------------- the float64 forward
def qkv_of(w, toks, pos0=0, dtype=np.float64):
    """q, k, v [B][H][T][64] of layer 0 for tokens toks [B][T] at positions pos0 .. pos0 + T - 1, from the stored weights w."""
    B, T = toks.shape
    E = w["wte"].shape[1]
    x = w["wte"][toks.astype(np.int64)] + w["wpe"][pos0:pos0 + T][None]
    a = sr.layernorm(x.reshape(B * T, E), w["h0.ln_1_g"], w["h0.ln_1_b"], dtype)
    y = a @ np.asarray(w["h0.c_attn_w"], dtype).T + np.asarray(w["h0.c_attn_b"], dtype)
    return tuple(y[:, i * E:(i + 1) * E].reshape(B, T, E // 64, 64).transpose(0, 2, 1, 3) for i in range(3))


def scores(q, K, past):
    """float64 scaled scores [B][H][n][T] of n queries behind `past` keys, -inf where a query does not see the key."""
    n, T = q.shape[2], K.shape[2]
    sc = np.einsum("bhqd,bhtd->bhqt", np.asarray(q, np.float64), np.asarray(K, np.float64)) * 0.125
    return np.where(np.arange(T)[None, :] <= past + np.arange(n)[:, None], sc, -np.inf)


def figures(sc):
    """Of scores [B][H][n][T]: the spread over the keys seen [B][H][n], the largest probability [B][H][n], the largest score."""
    top = sc.max(axis=-1)
    low = np.where(np.isfinite(sc), sc, np.inf).min(axis=-1)
    p = np.exp(sc - top[..., None])
    return top - low, 1.0 / p.sum(axis=-1), top


def conditions(regime, sc, past=0):
    """The regime's conditions on float64 scores sc [B][H][n][T] (n = 1: a decode step): a list of what does not hold."""
    name, hot = parse(regime)
    spread, pmax, top = figures(sc)
    bad = []
    if name == "trained":
        widest = spread.max(axis=-1)  # a head's widest row (the first query of a prompt sees one key: spread 0)
        if not (widest >= SPREAD[0]).all() or not (widest <= SPREAD[1]).all():
            bad.append(f"trained: score spread per head {widest.min():.1f} .. {widest.max():.1f}, not within {SPREAD}")
    elif name == "one-key":
        rows = past + np.arange(sc.shape[2]) >= hot  # the queries that see position `hot`
        rest = np.exp(sc[:, :, rows] - sc[:, :, rows, hot][..., None])
        rest[..., hot] = 0.0
        others = rest.sum(axis=-1)[:, 0]  # head 0 of every sequence, every such query
        if not rows.any() or not (others <= ONE_KEY_MASS).all():
            bad.append(f"one-key: the keys other than {hot} hold up to {others.max() if rows.any() else np.nan:.2e} of the mass, more than 2^-24")
    else:
        if not (top[:, 0] <= FAR_BELOW).all():
            bad.append(f"far-below: head 0's largest score {top[:, 0].max():.1f} is above {FAR_BELOW}")
    return bad


def describe(sc):
    spread, pmax, top = figures(sc)
    return f"score spread {spread.max(axis=-1).min():.1f} .. {spread.max():.1f}, largest probability {pmax.max():.9f}, scores {np.where(np.isfinite(sc), sc, np.inf).min():.1f} .. {top.max():.1f}"


# ---------------------------------------------------------------------------------------------- a float32 split kernel, and four ways to break it
def emulated(q, K, V, past, chunk=256, defect=None):
    """Causal attention as a split kernel evaluates it, in float32: scores as a float32 product, every `chunk` keys a split with its
    own maximum m, sum l and unnormalised o, the splits merged with w_s = exp(m_s - max m).  q [B][H][n][64], K / V [B][H][T][64].
    defect: "two planes" (the query cut to hi + mid in the score product), "scores b24" (scores rounded to 16 mantissa bits),
    "max from 0" (the running maximum started at 0 instead of -inf), "merge from first" (w_s = exp(m_s - m of the first split))."""
    f = np.float32
    q, K, V = (np.asarray(t, f) for t in (q, K, V))
    n, T = q.shape[2], K.shape[2]
    qs = sr.split3(q)[:2].sum(axis=0, dtype=f) if defect == "two planes" else q
    sc = np.einsum("bhqd,bhtd->bhqt", qs, K) * f(0.125)
    if defect == "scores b24":
        sc = sr.round_b24(sc)
    sc = np.where(np.arange(T)[None, :] <= past + np.arange(n)[:, None], sc, f(-np.inf))
    parts = []
    with np.errstate(all="ignore"):
        for t0 in range(0, T, chunk):
            s = sc[..., t0:t0 + chunk]
            m = s.max(axis=-1)
            if defect == "max from 0":
                m = np.maximum(m, f(0))
            p = np.exp(s - np.where(np.isfinite(m), m, f(0))[..., None])
            parts.append((np.einsum("bhqt,bhtd->bhqd", p, V[:, :, t0:t0 + chunk]), m, p.sum(axis=-1, dtype=f)))
        o, m, l = (np.stack(t, axis=-1) for t in zip(*parts))  # o [B][H][n][64][S], m / l [B][H][n][S]
        ref = m[..., :1] if defect == "merge from first" else m.max(axis=-1, keepdims=True)
        wgt = np.exp(m - ref)  # (a split a query sees nothing of: m = -inf, weight 0)
        return (o * wgt[..., None, :]).sum(axis=-1, dtype=f) / (wgt * l).sum(axis=-1, dtype=f)[..., None]


DEFECTS = ("two planes", "scores b24", "max from 0", "merge from first")


def worst(got, ref, s, rel=0.0):
    """stage_ref.metric_granted, with an output that is not finite counted as infinitely far off."""
    got = np.asarray(got, np.float64)
    return np.inf if not np.isfinite(got).all() else sr.metric_granted(got, ref, np.where(s > 0, s, 1e-300), rel)


# ---------------------------------------------------------------------------------------------- the attention's bound under a regime
def granted_outputs(regime, H, n, past):
    """[H][n] bools: the outputs (head, query) a regime hands to one key or puts far below 0 — held with stage_ref.ATTN_ULPS
    granted; every other output keeps the plain rule."""
    name, hot = parse(regime)
    mask = np.zeros((H, n), bool)
    if name == "one-key":
        mask[0] = past + np.arange(n) >= hot
    elif name == "far-below":
        mask[0] = True
    return mask


def attention_checks(regime, got, ref, s, y32, past, grant=sr.ATTN_ULPS, wide=3.0):
    """got / ref / s / y32 [B][H][n][64] -> [(what, worst, bound, Y)].  Without a regime and under `trained`: one entry, the
    project's rule (3 Y, Y the float32 numpy evaluation's own worst).  Under one-key / far-below the outputs granted_outputs names are
    measured with `grant` of the output granted on both sides, the others by the plain rule.  wide: the factor in place of 3 for the
    outputs whose scores the regime makes wide or large (all under `trained`, the granted ones under far-below), where the route
    has an entry in stage_ref.BOUND_Y."""
    name = parse(regime)[0]
    got, y32 = np.asarray(got, np.float64), np.asarray(y32, np.float64)
    B, H, n, _ = ref.shape
    mask = granted_outputs(regime, H, n, past)
    pick = lambda t, m: t[:, m]  # [B][outputs][64]
    out = []
    if (~mask).any():
        Y = sr.metric(pick(y32, ~mask), pick(ref, ~mask), pick(s, ~mask))
        out.append(("" if not mask.any() else "outputs the regime leaves alone", worst(pick(got, ~mask), pick(ref, ~mask), pick(s, ~mask)), (wide if name == "trained" else 3.0) * Y, Y))
    if mask.any():
        Y = worst(pick(y32, mask), pick(ref, mask), pick(s, mask), grant)
        out.append((f"{parse(regime)[0]} outputs, {grant * 2.0 ** 23:.0f} ulp of the output granted on both sides", worst(pick(got, mask), pick(ref, mask), pick(s, mask), grant), (wide if name == "far-below" else 3.0) * Y, Y))
    return out


def teeth(what, regime, q, K, V, past, chunk, wide=3.0):
    """The unbroken emulation and the four defects on float32 operands under attention_checks' bounds, the granted outputs with a
    grant half as wide again: {None or defect: it exceeds the bound of some check by half (and is not within the grant alone)}.
    Prints every figure."""
    q, K, V = (np.asarray(t, np.float32) for t in (q, K, V))
    ref, s = sr.causal_attention(q, K, V, past)
    y32 = sr.causal_attention(q, K, V, past, np.float32)[0]
    bites = {}
    for defect in (None,) + DEFECTS:
        got = emulated(q, K, V, past, chunk, defect)
        checks = attention_checks(regime, got, ref, s, y32, past, grant=sr.ATTN_ULPS * (1.0 if defect is None else 1.5), wide=wide)
        bites[defect] = any(w >= 1.5 * b and w > 0 for _, w, b, _ in checks)
        print(f"TEETH {what} | {defect or 'the emulation as it is'}: " + "; ".join(f"{name or 'all outputs'}: Y {Y:.2e} worst {w:.2e} = {w / b if b else (np.inf if w else 0.0):.2f} x the bound" for name, w, b, Y in checks))
        if defect is None:
            assert all(w <= b for _, w, b, _ in checks), (what, checks)  # the bounds pass a float32 split kernel that is not broken
    return bites
