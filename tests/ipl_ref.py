"""Python twin of include/fl_compat/ipl.h: the host state of slimIPL restated from recipes/slimIPL/src/Train.cpp -- the order of
supervised / unsupervised updates (:1214-1225, :1329-1333), the unsupervised batch of a step (:1238-1327), which samples have
labels and when the teacher labels (:1556-1609, :1786-1788, :1833-1840), the cache files (:490-545, :718-746).  Every random draw
comes from one splitmix64 stream seeded with --seed (the header's comment spells the stream, the uniform draw and the
Fisher-Yates shuffle out).  `scenario` replays a scripted run and returns the decisions as lines; tests/cpp/ipl_test.cpp prints
the same lines from the C++ class."""
import os

M64 = (1 << 64) - 1
TYPES = ("naive", "cache", "pre-cache", "fixed-pre-cache")


class Rng:
    def __init__(self, seed):
        self.state = seed & M64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def uniform(self):
        return (self.next() >> 11) * (1.0 / 9007199254740992.0)

    def shuffle(self, v):
        for i in range(len(v) - 1, 0, -1):
            j = self.next() % (i + 1)
            v[i], v[j] = v[j], v[i]


class SlimIPL:
    def __init__(self, type_, sup_updates, unsup_updates, fixed_cache_updates, fixed_cache_update_prob, n_unsup, seed):
        if type_ not in TYPES:
            raise ValueError(f"--slimIPL_type={type_}: expected naive | cache | pre-cache | fixed-pre-cache")
        if sup_updates < 0 or unsup_updates < 0 or sup_updates + (unsup_updates if n_unsup > 0 else 0) <= 0:
            raise ValueError("--slimIPL_sup_updates / --slimIPL_unsup_updates: negative, or no update of either kind")
        self.type, self.sup, self.unsup, self.U, self.prob, self.n = type_, sup_updates, unsup_updates, fixed_cache_updates, fixed_cache_update_prob, n_unsup
        self.fixed = type_ == "fixed-pre-cache"
        self.rng = Rng(seed)
        self.walk = list(range(max(0, n_unsup)))
        self.walk_idx, self.order, self.order_idx, self.to_label, self.cache_hits, self.snapshot = 0, [], 0, -1, 0, []
        self.pl_cache, self.pl_cache_dump, self.fixed_cache = {}, {}, []

    def begin(self):
        self.cache_hits = min(len(self.fixed_cache), self.U)
        if self.fixed and len(self.fixed_cache) >= self.U:
            self.rng.shuffle(self.fixed_cache)
            self.snapshot = list(self.fixed_cache)

    def start_epoch(self):
        if self.n > 0:
            if not self.fixed:
                self.walk = list(range(self.n))
            self.rng.shuffle(self.walk)
        self.walk_idx = 0
        self.order = [True] * self.sup + [False] * (self.unsup if self.n > 0 else 0)
        self.order_idx = 0
        self.rng.shuffle(self.order)

    def next_is_sup(self):
        return self.order[self.order_idx]

    def advance_order(self):
        self.order_idx += 1
        if self.order_idx >= len(self.order):
            self.order_idx = 0
            self.rng.shuffle(self.order)

    def next_unsup(self):
        """-> (train_batch or -1, label_next or -1, position, relabel)"""
        if not self.fixed:
            pos, b = self.walk_idx, self.walk[self.walk_idx % self.n]
            self.walk_idx += 1
            if self.walk_idx >= self.n:
                self.walk_idx = 0
                self.walk = list(range(self.n))
                self.rng.shuffle(self.walk)
            return b, -1, pos, True
        r = self.rng.uniform()
        relabel = len(self.fixed_cache) < self.U or r < self.prob
        if relabel:
            self.to_label += 1
        if self.to_label < 0 or self.to_label >= self.n:
            self.to_label = 0
            self.rng.shuffle(self.walk)
        if self.cache_hits == self.U:
            self.cache_hits = 0
            self.rng.shuffle(self.fixed_cache)
            self.snapshot = list(self.fixed_cache)
        pos, train = self.cache_hits, -1
        if len(self.fixed_cache) >= self.U:
            train = self.snapshot[self.cache_hits % len(self.snapshot)]
            if relabel:
                self.fixed_cache[self.cache_hits] = self.walk[self.to_label]
        else:
            self.fixed_cache.append(self.walk[self.to_label])
        nxt = self.walk[self.to_label] if relabel else -1
        self.cache_hits += 1
        return train, nxt, pos, relabel

    def labelled(self, ids):
        """-> (rows, texts, reused ids)"""
        reused = []
        for i in ids:
            if i not in self.pl_cache and i in self.pl_cache_dump:
                self.pl_cache[i] = self.pl_cache_dump[i]
                reused.append(i)
        rows = [k for k, i in enumerate(ids) if i in self.pl_cache]
        return rows, [self.pl_cache[ids[k]] for k in rows], reused

    def label_before_update(self, n_labelled):
        return self.type == "pre-cache" or (self.type != "naive" and n_labelled == 0)

    def label_after_update(self):
        return self.type == "cache"

    def store(self, ids, texts):
        for i, t in zip(ids, texts):
            self.pl_cache[i] = t

    # ---- files
    @staticmethod
    def _clean(t):
        return t.replace("|", " ").replace("\n", " ").replace("\r", " ")

    def cache_text(self):
        return "".join(f"{k}|{self._clean(self.pl_cache[k])}\n" for k in sorted(self.pl_cache, key=lambda s: s.encode()))

    def save_cache(self, path):
        with open(path, "w", encoding="utf-8", newline="") as f:
            f.write(self.cache_text())

    def load_cache_dump(self, path):
        if not os.path.exists(path):
            return -1
        n = 0
        with open(path, encoding="utf-8", newline="") as f:
            for line in f.read().split("\n"):
                if not line or line.startswith("|"):
                    continue
                parts = line.split("|")
                self.pl_cache_dump[parts[0]] = parts[1] if len(parts) > 1 else ""
                n += 1
        return n

    def fixed_cache_text(self):
        return "".join(f"{v} " for v in self.fixed_cache)

    def save_fixed_cache(self, path):
        with open(path, "w") as f:
            f.write(self.fixed_cache_text())

    def load_fixed_cache(self, path):
        if not os.path.exists(path):
            return False
        for tok in open(path).read().split():
            if len(self.fixed_cache) >= self.U:
                break
            v = int(tok)
            if v < 0 or v >= self.n:
                raise ValueError(f"{path}: batch index {v} outside the unsupervised list")
            self.fixed_cache.append(v)
        return True

    def state(self):
        v = [self.rng.state, self.order_idx, self.walk_idx, self.to_label, self.cache_hits, len(self.order)] + [int(b) for b in self.order]
        v += [len(self.walk)] + self.walk + [len(self.snapshot)] + self.snapshot
        return " ".join(str(x) for x in v)

    def set_state(self, text):
        t = [int(x) for x in text.split()]
        self.rng.state, self.order_idx, self.walk_idx, self.to_label, self.cache_hits, n = t[:6]
        self.order = [bool(b) for b in t[6:6 + n]]
        k = 6 + n
        n = t[k]
        if n != len(self.walk):
            raise ValueError("slimIPL state: written for another unsupervised list")
        self.walk = t[k + 1:k + 1 + n]
        k += 1 + n
        n = t[k]
        self.snapshot = t[k + 1:k + 1 + n]
        if len(self.snapshot) != n:
            raise ValueError("slimIPL state: malformed")


def scenario(type_, sup, unsup, n_unsup, U, prob, seed, steps=40, sup_per_epoch=4, per_batch=2):
    """A scripted run: `sup_per_epoch` supervised batches make an epoch, every unsupervised batch b holds the samples
    s<b>_<k>, and the "teacher" labels sample k of batch b at step t with the text `w<b> x<k> t<t>` (a trailing `'` when it labels
    after the update).  One line per decision."""
    ipl = SlimIPL(type_, sup, unsup, U, prob, n_unsup, seed)
    ipl.begin()
    out = []
    need, sup_in = True, 0
    ids = lambda b: [f"s{b}_{k}" for k in range(per_batch)]
    teacher = lambda b, t, mark="": [f"w{b} x{k} t{t}{mark}" for k in range(per_batch)]
    for t in range(1, steps + 1):
        if need:
            ipl.start_epoch()
            need = False
            out.append(f"{t} epoch")
        if ipl.next_is_sup():
            ipl.advance_order()
            out.append(f"{t} sup")
            sup_in += 1
            if sup_in == sup_per_epoch:
                need, sup_in = True, 0
            continue
        train, nxt, pos, relabel = ipl.next_unsup()
        ipl.advance_order()
        rows, texts, to_save = [], [], None
        if type_ == "naive":
            texts = teacher(train, t)
            rows = list(range(per_batch))
        else:
            if train >= 0:
                rows, texts, _ = ipl.labelled(ids(train))
                if ipl.label_before_update(len(rows)):
                    to_save = teacher(train, t)
            if nxt >= 0:
                ipl.store(ids(nxt), teacher(nxt, t))
        if to_save is not None:
            ipl.store(ids(train), to_save)
        if train >= 0 and ipl.label_after_update():
            ipl.store(ids(train), teacher(train, t, "'"))
        out.append(f"{t} unsup train={train} pos={pos} relabel={int(relabel)} next={nxt} rows={','.join(map(str, rows))} "
                   f"texts={';'.join(texts)} update={int(len(rows) > 0)}")
    out.append("cache " + ipl.cache_text().replace("\n", "/"))
    out.append("fixed " + ipl.fixed_cache_text())
    out.append("state " + ipl.state())
    return out


def scenarios():
    """H1: all four types; sup:unsup 1:3 and 0:1; 3 and 7 unsupervised batches; fixed_cache_updates 2 and 5; update probability
    0, 0.5 and 1 -- 40 steps each"""
    s = []
    for type_ in TYPES:
        for sup, unsup in ((1, 3), (0, 1)):
            for n_unsup in (3, 7):
                for U, prob in (((2, 0.0), (2, 0.5), (2, 1.0), (5, 0.0), (5, 0.5), (5, 1.0)) if type_ == "fixed-pre-cache" else ((2, 1.0),)):
                    s.append((type_, sup, unsup, n_unsup, U, prob, 7 + len(s)))
    return s


def expected_log(type_, sup, unsup, n_unsup, U, prob, seed, steps, sup_per_epoch):
    """What `Train` logs for a run from scratch whose unsupervised batches are labelled as wholes: per update "sup", "unsup <position>"
    (fixed-pre-cache: "unsup <position> <update cache 0|1>") or "notready", followed by "skip" when the update has no label to train
    on.  Also returns the unsupervised batches that hold labels at the end and the fixed cache."""
    ipl = SlimIPL(type_, sup, unsup, U, prob, n_unsup, seed)
    ipl.begin()
    out, labelled = [], set()
    need, sup_in = True, 0
    for _ in range(steps):
        if need:
            ipl.start_epoch()
            need = False
        if ipl.next_is_sup():
            ipl.advance_order()
            out.append("sup")
            sup_in += 1
            if sup_in == sup_per_epoch:
                need, sup_in = True, 0
            continue
        train, nxt, pos, relabel = ipl.next_unsup()
        ipl.advance_order()
        out.append("notready" if train < 0 else (f"unsup {pos} {int(relabel)}" if type_ == "fixed-pre-cache" else f"unsup {pos}"))
        have = type_ == "naive" or train in labelled
        if train >= 0 and type_ != "naive" and (type_ in ("cache", "pre-cache") or not have):
            labelled.add(train)      # labelled before (pre-cache, or nothing to train on) or after (cache) the update
        if nxt >= 0:
            labelled.add(nxt)
        if not have:
            out.append("skip")
    return out, sorted(labelled), list(ipl.fixed_cache)
