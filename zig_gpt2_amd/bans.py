"""History-dependent token bans on the host (include/zgpt2.h zg_ban_rules): the twin of the device loop's ban stage
for callers who draw token by token.  There is no per-token C entry: pass `banned_now(...)` as `banned_token_ids` of GPT.sample /
GPT.sample_each, together with whatever the call bans statically."""
from . import _lib

MAX_NGRAM, MAX_WORDS, MAX_WORD_LEN, MAX_SUPPRESS = _lib.BAN_MAX_NGRAM, _lib.BAN_MAX_WORDS, _lib.BAN_MAX_WORD_LEN, _lib.BAN_MAX_SUPPRESS


def banned_now(history, picked, n=0, words=None, min_tokens=0, suppress_ids=None, vocab=None):
    """The sorted token ids forbidden for the next pick of a row whose history — prior, prompt and picks so far, in order — is
    `history` and which has made `picked` picks (negative: the row is still in its prompt).
    n: no_repeat_ngram_size (0: off) — every token that would complete an n-gram the history already holds.
    words: bad words as token-id lists — the last token of a word while the history ends in the tokens before it.
    min_tokens / suppress_ids: the ids that cannot be picked while 0 <= picked < min_tokens.
    vocab (optional): a history token >= vocab matches nothing and bans nothing, as on the device."""
    h = [int(t) for t in history]
    words = [[int(t) for t in w] for w in (words or [])]
    suppress_ids = [int(t) for t in (suppress_ids if suppress_ids is not None else [])]
    if not 0 <= n <= MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size {n} outside 0..{MAX_NGRAM}")
    if len(words) > MAX_WORDS or any(not 1 <= len(w) <= MAX_WORD_LEN for w in words):
        raise ValueError(f"bad words: at most {MAX_WORDS} words of 1..{MAX_WORD_LEN} tokens")
    if len(suppress_ids) > MAX_SUPPRESS:
        raise ValueError(f"{len(suppress_ids)} suppress ids above {MAX_SUPPRESS}")
    if vocab is not None:  # (a token outside the vocabulary can equal nothing: -1 never occurs in a word, and kills an n-gram below)
        h = [t if 0 <= t < vocab else -1 for t in h]
    L = len(h)
    out = set()
    if n >= 1 and L >= n - 1:
        tail = h[L - n + 1:]
        if -1 not in tail:
            for i in range(L - n + 1):
                if h[i: i + n - 1] == tail and h[i + n - 1] != -1:
                    out.add(h[i + n - 1])
    for w in words:
        m = len(w)
        if L >= m - 1 and h[L - m + 1:] == w[: m - 1]:
            out.add(w[-1])
    if 0 <= picked < min_tokens:
        out.update(suppress_ids)
    return sorted(out)
