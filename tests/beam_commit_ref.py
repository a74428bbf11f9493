"""The commit rule of w2l_beam_session_commit restated in numpy over the existing reference searches, and the inputs shared by
test_beam_commit_host.py and test_gpu_beam_commit.py.

The rule: take the prefixes of ALL live beam entries; their longest common prefix less its last label is committed (that label
stays in the table, so no entry is left at the root with a real last label); every row splits into the committed part and a tail;
the rebuilt table holds the distinct non-empty prefixes of the tails.

The inputs.  A beam forgets an old alternative only when enough cheaper ones displace it (its distance to the best hypothesis
never changes afterwards, whatever the threshold), so stationary emissions let a wide beam keep an early near-tie for hundreds of
frames.  `ramped` is beam_stream_cases.peaked's picture -- runs of 1-3 frames with one class on top, a runner-up and the blank close
behind, a background far below, all multiples of 1/8 -- with two changes: the blank is never level with the top class (a permanent
tie would stay in every beam), and frame t is scaled by a power of two that halves every `halve` frames, so later alternatives are
cheaper than earlier ones and displace them.  Sums stay exact in fp32 (|x| < 2^16)."""
import functools

import numpy as np

from tests import beam_stream_cases as BC
from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as R

F32 = np.float32
INF = float("inf")


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def lcp(prefixes):
    """length of the longest common prefix of all the tuples (0 for none)"""
    prefixes = list(prefixes)
    if not prefixes:
        return 0
    n = min(len(p) for p in prefixes)
    first = prefixes[0]
    for i in range(n):
        if any(p[i] != first[i] for p in prefixes):
            return i
    return n


def commit_len(prefixes):
    """labels committed in total once a commit has seen these live prefixes: max(0, LCP - 1)"""
    return max(0, lcp(prefixes) - 1)


def split(row, done):
    """a row (tuple) into its committed part and its tail"""
    return tuple(row[:done]), tuple(row[done:])


def live_nodes(prefixes, done):
    """nodes of the rebuilt table: the distinct non-empty prefixes of the tails"""
    return len({p[done:k] for p in prefixes for k in range(done + 1, len(p) + 1)})


def budget(live, beam, max_frames):
    """frames a slot may take after a commit that left `live` nodes"""
    return max_frames - (live + beam - 1) // beam


# ---- the live prefixes, by the existing references ---------------------------------------------------------------------------
def live_prefixes(x, F, W, K, threshold=INF, log_add=False, normalize=False, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0):
    """prefixes of every beam entry after F frames (LM-free, or with a token LM: the end-of-sentence term reorders rows, it drops
    none)"""
    if F == 0:
        return [()]
    if lm is None:
        hyps, _ = R.beam_search_one(x, F, W, K, threshold, log_add, normalize, F32, None)
    else:
        hyps, _ = LR.beam_search_lm_one(x, F, W, K, lm, lm_weight, class_score, eos_score, threshold, log_add, normalize, F32, None)
    return [h[0] for h in hyps]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def ramped(rng, T, N, halve=3):
    x = (rng.integers(-40, -15, size=(T, N)) / 8).astype(F32)
    t = 0
    while t < T:
        run = int(rng.integers(1, 4))
        c, c2 = int(rng.integers(0, N - 1)), int(rng.integers(0, N - 1))
        for u in range(t, min(t + run, T)):
            x[u, c2] = -rng.integers(1, 8) / 8
            x[u, N - 1] = -rng.integers(1, 6) / 8
            x[u, c] = 0.0
        t += run
    scale = np.array([2.0 ** ((T - 1 - t) // halve) for t in range(T)], F32)
    return (x * scale[:, None]).astype(F32)


def spelled(rng, T, N, trie, halve=3):
    """`ramped` for the lexicon search, whose beam can only follow words: the top classes spell words of the lexicon, in runs of 1-3
    frames, the silence token between two words now and then, a blank frame between two equal tokens.  Two hypotheses that differ in the choice
    between homophones, or in where one word ends and the next begins (silence is optional, and a spelling may hold the silence
    token), differ by LM terms alone, which the ramp does not scale: such pairs would stay in every beam for good.  So a word is
    appended only if the labels so far keep ONE derivation (TextbookTrie.derivations)."""
    spellings = [tuple(sp) for _, sp in trie.rows]
    words = sorted({sp for sp in spellings if len(trie.derivations(sp)) == 1}, key=lambda sp: (len(sp), sp))[:24]
    assert words, "no word with one reading"
    chosen, tries = [], 0          # [(labels so far, words not yet tried behind them)]; bounded: a search that fails says so
    while not chosen or len(chosen[-1][0]) < T:
        tries += 1
        assert tries < 4000, "no utterance with one reading found"
        if not chosen:
            chosen.append(((), None))
        tokens, left = chosen[-1]
        if left is None:
            left = [(sep, words[int(j)]) for j in rng.permutation(len(words)) for sep in (((trie.sil,), ()) if tokens else ((),))]
        while left:
            sep, sp = left.pop()
            if len(trie.derivations(tokens + sep + sp)) == 1:
                chosen[-1] = (tokens, left)
                chosen.append((tokens + sep + sp, None))
                break
        else:
            chosen.pop()            # a dead end: every continuation has a second reading; take the last word back
    tokens = chosen[-1][0]
    x = (rng.integers(-40, -15, size=(T, N)) / 8).astype(F32)
    t, last = 0, None
    for c in tokens:
        if t >= T:
            break
        if c == last:               # the same token again: a frame of blank keeps the two apart
            x[t, N - 1] = 0.0
            x[t, c] = -rng.integers(1, 8) / 8
            t += 1
        c2 = int(rng.integers(0, N - 1))
        for u in range(t, min(t + int(rng.integers(1, 4)), T)):
            x[u, c2] = -rng.integers(1, 8) / 8
            x[u, N - 1] = -rng.integers(1, 6) / 8
            x[u, c] = 0.0
            t = u + 1
        last = c
    scale = np.array([2.0 ** ((T - 1 - t) // halve) for t in range(T)], F32)
    return (x * scale[:, None]).astype(F32)


T = 40
MAX_CHUNK = 3
MAX_FRAMES_B, MAX_FRAMES_A = 8, 64
PATTERN = (1, 2, 0, 3, 2, 1, 3, 0)     # frames per step, by the step's number: chunks of 0 to 3, and two steps carry 3 frames at most
COMMIT_EVERY = 2                        # a commit after every 2nd step
LATE, RESET_AT, AGAIN = 3, 12, 14       # slot 0 starts at step LATE; slot 1 starts at step 0, is reset after step RESET_AT - 1 and
#                                         starts anew at step AGAIN; slot 2 never starts


@functools.lru_cache(maxsize=None)
def utterances(N, lex=False):
    """slot 0's utterance, slot 1's first (cut short by the reset) and its second; lex: spelled from the stream tests' lexicon"""
    rng = np.random.default_rng(7000 + 10 * N + (1 if lex else 0))
    if not lex:
        return ramped(rng, T, N), ramped(rng, T, N), ramped(rng, T, N)
    trie, _ = BC.lexicon_and_word_lm(N)
    return tuple(spelled(rng, T, N, trie) for _ in range(3))


def schedule(N, lex=False):
    """steps of the three-slot session: (emissions [3][MAX_CHUNK][N], n [3], start [3], reset: slots closed BEFORE the step,
    commit: whether a commit follows the step, fed: per slot (utterance index or None, frames it has had after the step))"""
    xs = utterances(N, lex)
    steps, pos, utt = [], [0, 0, 0], [None, None, None]
    i = 0
    while True:
        em = np.zeros((3, MAX_CHUNK, N), F32)
        n, st, reset = np.zeros(3, np.int32), np.zeros(3, np.int32), []
        c = PATTERN[i % len(PATTERN)]
        if i == LATE:
            utt[0], pos[0], st[0] = 0, 0, 1
        if i == 0:
            utt[1], pos[1], st[1] = 1, 0, 1
        if i == RESET_AT:
            reset.append(1)
            utt[1] = None
        if i == AGAIN:
            utt[1], pos[1], st[1] = 2, 0, 1
        for s in (0, 1):
            if utt[s] is not None:
                k = min(c, T - pos[s])
                em[s, :k] = xs[utt[s]][pos[s]:pos[s] + k]
                n[s] = k
                pos[s] += k
        steps.append((em, n, st, reset, i % COMMIT_EVERY == COMMIT_EVERY - 1, [(utt[s], pos[s]) for s in range(3)]))
        i += 1
        if i > AGAIN and all(utt[s] is None or pos[s] == T for s in (0, 1)):
            return steps


def simulate(x, feed, W, K, max_frames, **search):
    """The rule over one slot's life.  feed: [(frames of the step, commit after it)].  Returns per step a dict: F (frames so far),
    done (labels committed so far), live (nodes after the last commit, None before the first), used (frames counted against
    max_frames after the step), and at the end the best row's length."""
    F = done = 0
    live, since, out = None, 0, []
    for n, commit in feed:
        F += n
        since += n
        used = since + (0 if live is None else (live + W - 1) // W)
        rec = dict(F=F, used=used, refused=used > max_frames)
        if commit:
            pre = live_prefixes(x, F, W, K, **search)
            done = max(done, commit_len(pre))
            live, since = live_nodes(pre, done), 0
        rec.update(done=done, live=live)
        out.append(rec)
    return out
