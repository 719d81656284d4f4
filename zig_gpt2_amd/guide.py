"""Token-level automata for guided decoding (include/zgpt2.h zg_guide) and three ways to build one.

A `Guide` is a dense table next [n_states, vocab] of uint16: DEAD where a state does not allow a token, else the state behind
picking it.  Every state allows at least one token ("done" is a state that loops on the end token; ending the generation is the
stop stage's business), and one table may hold several automata in disjoint state ranges (`Guide.union`): every row of a
generation names its own start state.  The rules are the library's own: a table is checked through zg_debug_guide_check, which
needs no GPU.  There is no regex parser here: `from_byte_dfa` lifts a byte-level DFA that the caller compiled by whatever means.
"""
import ctypes as C

import numpy as np

from . import _lib

DEAD = _lib.GUIDE_DEAD
NONE = _lib.GUIDE_NONE
MAX_STATES = _lib.GUIDE_MAX_STATES


class Guide:
    def __init__(self, next):
        """next: [n_states, vocab] integers, DEAD (0xFFFF) or a state < n_states.  ValueError where the library would refuse it."""
        a = np.asarray(next)
        if a.ndim != 2 or a.shape[1] < 1:
            raise ValueError(f"a guide is a table [n_states, vocab], not {a.shape}")
        if a.size and (a.min() < 0 or a.max() > DEAD):
            raise ValueError("a transition outside uint16")
        self.next = np.ascontiguousarray(a, dtype=np.uint16)
        rc = _lib.load().zg_debug_guide_check(C.addressof(self.c_struct()), self.vocab, None, None, 0, 0)
        if rc != 0:
            raise ValueError(_lib.load().zg_last_error().decode(errors="replace"))

    @property
    def n_states(self):
        return self.next.shape[0]

    @property
    def vocab(self):
        return self.next.shape[1]

    def c_struct(self):
        """zg_guide over this table (the table must stay alive while the structure is in use)."""
        return _lib.Guide(self.n_states, _lib.ptr(self.next))

    def allowed(self, state):
        """The token ids state `state` allows, ascending."""
        return np.flatnonzero(self.next[state] != DEAD)

    def step(self, state, token):
        """The state behind picking `token` in `state` (ValueError where it is not allowed)."""
        nx = int(self.next[state, token])
        if nx == DEAD:
            raise ValueError(f"state {state} does not allow token {token}")
        return nx

    def walk(self, state, tokens):
        """The state behind picking `tokens` in turn, starting from `state`."""
        for t in tokens:
            state = self.step(state, int(t))
        return state

    # ------------------------------------------------------------------ builders
    @classmethod
    def from_choices(cls, token_sequences, vocab, end_token):
        """ "Answer with one of these": a trie over the token sequences, start state 0.  Behind the last token of a choice the row
        is done — the last state, which allows end_token alone and loops on it; a choice that is also the prefix of a longer one
        allows end_token beside the longer one's next token.  Multi-token labels, which a static allow-list cannot express."""
        seqs = [[int(t) for t in q] for q in token_sequences]
        if not seqs or any(len(q) == 0 for q in seqs):
            raise ValueError("from_choices: no choices, or an empty one")
        if any(t == end_token for q in seqs for t in q) or not 0 <= end_token < vocab:
            raise ValueError("from_choices: end_token inside a choice, or outside the vocabulary")
        if any(not 0 <= t < vocab for q in seqs for t in q):
            raise ValueError("from_choices: a token outside the vocabulary")
        full = {tuple(q) for q in seqs}
        inner = {()}  # prefixes that something follows: the states of the trie
        for q in seqs:
            inner.update(tuple(q[:i]) for i in range(1, len(q)))
        order = sorted(inner, key=lambda p: (len(p), p))
        index = {p: i for i, p in enumerate(order)}
        done = len(order)
        if done + 1 > MAX_STATES:
            raise ValueError(f"from_choices: {done + 1} states above {MAX_STATES}")
        nxt = np.full((done + 1, vocab), DEAD, np.uint16)
        for q in seqs:
            for i, t in enumerate(q):
                after = tuple(q[: i + 1])
                nxt[index[tuple(q[:i])], t] = index[after] if after in inner else done
        for p in full & inner:  # a whole choice that a longer one continues
            nxt[index[p], end_token] = done
        nxt[done, end_token] = done
        return cls(nxt)

    @classmethod
    def from_byte_dfa(cls, trans, start, accepting, token_bytes, end_token):
        """Lift a byte-level DFA to tokens.  trans [S, 256]: the state behind a byte, negative (or >= S) where the byte is not
        allowed; token_bytes: the bytes of every token id (len(token_bytes) is the vocabulary; end_token's are not read).  From a
        state a token is allowed iff walking its bytes survives (a token of no bytes never is), and leads where the walk ends;
        end_token is allowed in accepting states and leads to a done state that loops on it.  Only states reachable over token
        transitions are kept, the start state as state 0.  ValueError if a reachable state allows nothing or more than 256 remain."""
        trans = np.asarray(trans, dtype=np.int64)
        S, vocab = trans.shape[0], len(token_bytes)
        if trans.ndim != 2 or trans.shape[1] != 256 or not 0 <= start < S or not 0 <= end_token < vocab:
            raise ValueError("from_byte_dfa: trans must be [S, 256], start a state, end_token a token")
        trans = np.where((trans < 0) | (trans >= S), -1, trans)
        accepting = {int(a) for a in accepting}
        lens = np.array([len(b) for b in token_bytes], np.int64)
        lens[end_token] = 0
        width = max(int(lens.max()), 1)
        mat = np.zeros((vocab, width), np.int64)
        for i, b in enumerate(token_bytes):
            if i != end_token and len(b):
                mat[i, : len(b)] = np.frombuffer(bytes(b), np.uint8)

        def lift(s):  # where every token leads from byte state s; -1: not allowed
            cur = np.where(lens > 0, s, -1)
            for j in range(width):
                live = (cur >= 0) & (lens > j)
                cur = np.where(live, trans[np.maximum(cur, 0), mat[:, j]], cur)
            return cur

        order, index, rows = [start], {start: 0}, []
        need_done = False
        for s in order:  # (grows while it is walked: breadth first)
            to = lift(s)
            for t in np.unique(to[to >= 0]):
                if int(t) not in index:
                    index[int(t)] = len(order)
                    order.append(int(t))
            rows.append(to)
            need_done = need_done or s in accepting
            if len(order) > MAX_STATES:
                break
        done = len(order)
        if done + int(need_done) > MAX_STATES:
            raise ValueError(f"from_byte_dfa: more than {MAX_STATES} reachable states")
        nxt = np.full((done + int(need_done), vocab), DEAD, np.uint16)
        remap = np.full(S + 1, DEAD, np.int64)
        for s, i in index.items():
            remap[s] = i
        for i, (s, to) in enumerate(zip(order, rows)):
            nxt[i] = remap[to]  # (-1 indexes the spare last entry: DEAD)
            if s in accepting:
                nxt[i, end_token] = done
            if not (nxt[i] != DEAD).any():
                raise ValueError(f"from_byte_dfa: byte state {s} is reachable and allows no token")
        if need_done:
            nxt[done, end_token] = done
        return cls(nxt)

    @staticmethod
    def union(guides):
        """One table holding every guide in its own state range: (Guide, [the offset of each guide's state 0])."""
        guides = list(guides)
        if not guides or len({g.vocab for g in guides}) != 1:
            raise ValueError("union: no guides, or guides over different vocabularies")
        offsets = [int(o) for o in np.cumsum([0] + [g.n_states for g in guides[:-1]])]
        if offsets[-1] + guides[-1].n_states > MAX_STATES:
            raise ValueError(f"union: {offsets[-1] + guides[-1].n_states} states above {MAX_STATES}")
        parts = [np.where(g.next == DEAD, DEAD, g.next.astype(np.int64) + o) for g, o in zip(guides, offsets)]
        return Guide(np.concatenate(parts)), offsets
