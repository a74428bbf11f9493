"""Lexicon: the lexicon trie of the lexicon-constrained CTC beam search (w2l_lexicon_*; the contract -- nodes, edges, the six words
of a node, smear, the blob -- is in include/w2l_hip.h).  The table is built and walked on the host by libw2l_hip.so;
device_blob() copies its bytes, unchanged, to the GPU for criterion.ctc_beam_search(..., lexicon=...)."""
import ctypes as C

import numpy as np

from . import _lib, text
from .lm import _aligned, _fail


class Lexicon:
    """words[i] spells word id i: the ranks of the words sorted bytewise (UTF-8), the list NGramLM.from_arpa(path, words) takes"""

    def __init__(self, blob, words=None, dropped=0):
        L = _lib.lib()
        self.blob = blob
        self.dropped = dropped
        v = [C.c_int() for _ in range(5)]
        st = L.w2l_lexicon_info(blob.ctypes.data, *[C.addressof(x) for x in v])
        if st:
            _fail(st, "Lexicon")
        self.num_tokens, self.num_words, self.num_nodes, self.sil = (x.value for x in v[:4])
        self.smeared = bool(v[4].value)
        self.words = list(words) if words is not None else [str(i) for i in range(self.num_words)]
        self._device = {}

    @classmethod
    def from_spellings(cls, spellings, num_tokens, num_words, word_smear=None, sil=None, words=None):
        """spellings: rows (word id, [token ids]) in the order that decides which six words a node keeps; word_smear: [num_words]
        float32 or None (no smearing); sil: the silence token or None"""
        L = _lib.lib()
        rows = [(int(w), [int(t) for t in sp]) for w, sp in spellings]
        sw = np.array([w for w, _ in rows], np.int32)
        off = np.zeros(len(rows) + 1, np.uintp)
        off[1:] = np.cumsum([len(sp) for _, sp in rows])
        toks = np.array([t for _, sp in rows for t in sp], np.int32)
        sm = None
        if word_smear is not None:
            sm = np.ascontiguousarray(word_smear, np.float32)
            if sm.shape != (int(num_words),):
                raise _lib.W2LInvalidArgument("Lexicon.from_spellings: word_smear must have one entry per word")
        dropped = C.c_size_t(0)

        def call(b, n):
            return L.w2l_lexicon_build(int(num_tokens), int(num_words), len(rows), sw.ctypes.data, off.ctypes.data, toks.ctypes.data,
                                       sm.ctypes.data if sm is not None else None, -1 if sil is None else int(sil), b, n,
                                       C.addressof(dropped))
        size = C.c_size_t(0)
        st = call(None, C.addressof(size))
        if st:
            _fail(st, "Lexicon.from_spellings")
        blob = _aligned(size.value)
        st = call(blob.ctypes.data, C.addressof(size))
        if st:
            _fail(st, "Lexicon.from_spellings")
        return cls(blob, words, dropped.value)

    @classmethod
    def from_file(cls, path, token_dict, lm=None, sil=None, smearing="max", replabel=0):
        """a lexicon file (text.load_lexicon: `word tok tok ...`, every spelling of a word a line) over token_dict (a
        text.Dictionary, or the list of token spellings).  sil: the spelling of the silence token, or None.  smearing "max":
        wordSmear[w] = lm.score(lm.start, w) (lm: the NGramLM over Lexicon.words); "none": no smearing.  replabel > 0 (an ASG
        model's --replabel): every spelling is packed with text.pack_replabels before the trie is built -- `h e l l o` becomes
        `h e l <1> o` -- and the tokens `<1>` .. `<replabel>` must be in token_dict"""
        if smearing not in ("max", "none"):
            raise _lib.W2LInvalidArgument(f"Lexicon.from_file: smearing {smearing!r} is not built: `max` or `none`")
        if not isinstance(token_dict, text.Dictionary):
            token_dict = text.Dictionary(list(token_dict))
        replabel = int(replabel)
        for r in range(1, replabel + 1):
            if not token_dict.contains(text.replabel_token(r)):
                raise _lib.W2LInvalidArgument(f"Lexicon.from_file: replabel={replabel} needs the token `{text.replabel_token(r)}` "
                                              "in the token dictionary")
        lex = text.load_lexicon(str(path))
        words = sorted(lex, key=lambda w: w.encode())
        wid = {w: i for i, w in enumerate(words)}
        rows = []
        for w, spellings in lex.items():                      # file order: the first six words of a node are the file's first
            for sp in spellings:
                for t in sp:
                    if not token_dict.contains(t):
                        raise _lib.W2LInvalidArgument(f"Lexicon.from_file: the spelling of `{w}` has the token `{t}`, which the token "
                                                      "dictionary lacks")
                rows.append((wid[w], text.pack_replabels([token_dict.get_index(t) for t in sp], token_dict, replabel)))
        smear = None
        if smearing == "max" and lm is not None:
            if lm.num_tokens != len(words):
                raise _lib.W2LInvalidArgument(f"Lexicon.from_file: the LM has {lm.num_tokens} words, the lexicon {len(words)}")
            smear = np.array([lm.score(lm.start, i)[0] for i in range(len(words))], np.float32)
        sil_id = None
        if sil is not None:
            if not token_dict.contains(sil):
                raise _lib.W2LInvalidArgument(f"Lexicon.from_file: the silence token `{sil}` is not in the token dictionary")
            sil_id = token_dict.get_index(sil)
        return cls.from_spellings(rows, token_dict.index_size(), len(words), smear, sil_id, words)

    def child(self, node, token):
        """the child of `node` by `token`, -1 when the edge is absent"""
        c = C.c_int()
        st = _lib.lib().w2l_lexicon_child(self.blob.ctypes.data, int(node), int(token), C.addressof(c))
        if st:
            _fail(st, "Lexicon.child")
        return c.value

    def node(self, node):
        """(smear as float32, [word ids], has_children)"""
        sm, nw, hc = C.c_float(), C.c_int(), C.c_int()
        w = (C.c_int * 6)()
        st = _lib.lib().w2l_lexicon_node(self.blob.ctypes.data, int(node), C.addressof(sm), C.addressof(nw), C.addressof(w), C.addressof(hc))
        if st:
            _fail(st, "Lexicon.node")
        return np.float32(sm.value), [w[i] for i in range(nw.value)], bool(hc.value)

    def device_blob(self, device):
        """the table on `device` (copied once per device)"""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = torch.from_numpy(np.array(self.blob)).to(device)
        return self._device[device]
