"""IMDB text pipeline (pytorch_on_language_distr.py:31-149).

* ``rm_tags`` / ``read_files`` — pandas CSV reader, ``sentiment == 'positive'`` -> 1, HTML tags
  stripped (the reference's regex);
* ``split_reference`` — first 10,000 reviews train, 10,000..12,500 test (B11);
* ``encode`` — the native multithreaded pipeline ``torch.ops.pcmp.text_encode`` (BERT
  basic+WordPiece tokenisation, [CLS]/[SEP], truncation and post-padding to 128, attention
  masks) with a pure-Python fallback of identical semantics;
* ``build_vocab`` — the bert-base-uncased vocabulary cannot be downloaded here, so a WordPiece
  vocabulary with BERT's special-token ids ([PAD]=0, [UNK]=100, [CLS]=101, [SEP]=102,
  [MASK]=103) is built from corpus word frequencies (plus single characters and their '##'
  forms, so every word tokenises); a real ``vocab.txt`` is used when one is given;
* ``train_val_split`` — sklearn ``train_test_split(random_state=2020, test_size=0.1)`` applied
  identically to ids, labels and masks (B15).
"""
from __future__ import annotations

import re
import string
from collections import Counter
from dataclasses import dataclass, replace

import torch

SPECIALS = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103}
_TAGS = re.compile(r"<[^>]+>")


def rm_tags(text):
    return _TAGS.sub(" ", text)


def read_files(path):
    import pandas as pd
    df = pd.read_csv(path)
    df["sentiment"] = (df["sentiment"] == "positive") * 1
    df["review"] = df["review"].apply(rm_tags)
    return df["review"].values, df["sentiment"].values


def split_reference(texts, labels):
    return (texts[:10000], labels[:10000]), (texts[10000:12500], labels[10000:12500])


def _native():
    from ..ops import _lib
    return _lib.load() and hasattr(torch.ops.pcmp, "text_encode")


_CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
        (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
_WS = {0x9, 0xA, 0xB, 0xC, 0xD, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F,
       0x3000}


def _is_punct(ch):
    import unicodedata
    cp = ord(ch)
    return (33 <= cp <= 47) or (58 <= cp <= 64) or (91 <= cp <= 96) or (123 <= cp <= 126) or \
        unicodedata.category(ch).startswith("P")


def _py_basic(text, lower=True, strip=True):
    """Pure-Python twin of the native basic tokenizer (csrc/runtime/text_core.h): HuggingFace
    BertNormalizer (clean text, isolate CJK ideographs, strip accents + lowercase) + BertPreTokenizer
    (whitespace split, punctuation isolated)."""
    import unicodedata
    if strip:
        text = rm_tags(text)
    buf = []
    for ch in text:
        cp = ord(ch)
        if ch in "\t\n\r":
            buf.append(" ")
            continue
        if cp == 0 or cp == 0xFFFD or unicodedata.category(ch)[0] == "C":
            continue
        if cp in _WS:
            buf.append(" ")
        elif any(lo <= cp <= hi for lo, hi in _CJK):
            buf.append(" " + ch + " ")
        else:
            buf.append(ch)
    text = "".join(buf)
    if lower:
        text = "".join(c.lower() for c in unicodedata.normalize("NFD", text) if unicodedata.category(c) != "Mn")
    out, cur = [], []
    for ch in text:
        if ch == " ":
            if cur:
                out.append("".join(cur)); cur = []
        elif _is_punct(ch):
            if cur:
                out.append("".join(cur)); cur = []
            out.append(ch)
        else:
            cur.append(ch)
    if cur:
        out.append("".join(cur))
    return out


def basic_tokenize(texts, lower=True, strip=True):
    texts = [str(t) for t in texts]
    if _native():
        return [s.split(" ") if s else [] for s in torch.ops.pcmp.text_basic_tokenize(texts, lower, strip)]
    return [_py_basic(t, lower, strip) for t in texts]


def build_vocab(texts, size=30522, lower=True):
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    chars = set()
    cnt = Counter()
    for toks in basic_tokenize(texts, lower):
        cnt.update(toks)
        for t in toks:
            chars.update(t)
    pieces = sorted(chars) + ["##" + c for c in sorted(chars)]
    seen = set(vocab)
    for p in pieces:
        if p not in seen:
            vocab.append(p); seen.add(p)
    for w, _ in cnt.most_common():
        if len(vocab) >= size:
            break
        if w not in seen:
            vocab.append(w); seen.add(w)
    return vocab


def load_vocab(path):
    with open(path, encoding="utf-8") as f:
        return [l.rstrip("\n") for l in f]


def _py_wordpiece(word, vmap, unk):
    if len(word) > 100:   # code points
        return [unk]
    out, start = [], 0
    while start < len(word):
        end, cur = len(word), None
        while start < end:
            sub = word[start:end]
            if start > 0:
                sub = "##" + sub
            if sub in vmap:
                cur = vmap[sub]
                break
            end -= 1
        if cur is None:
            return [unk]
        out.append(cur)
        start = end
    return out


def encode(texts, vocab, max_len=128, lower=True, strip=True, force_python=False):
    """-> (input_ids int64 [N,max_len], attention_mask int64 [N,max_len])."""
    texts = [str(t) for t in texts]
    if _native() and not force_python:
        ids, mask = torch.ops.pcmp.text_encode(texts, list(vocab), max_len, lower, strip)
        return ids, mask
    vmap = {w: i for i, w in enumerate(vocab)}
    unk, cls, sep = vmap.get("[UNK]", 100), vmap.get("[CLS]", 101), vmap.get("[SEP]", 102)
    ids = torch.zeros(len(texts), max_len, dtype=torch.long)
    for n, t in enumerate(texts):
        wp = []
        for tok in _py_basic(t, lower, strip):
            wp += _py_wordpiece(tok, vmap, unk)
            if len(wp) >= max_len:
                break
        row = [cls] + wp[: max_len - 2] + [sep]
        ids[n, : len(row)] = torch.tensor(row)
    return ids, (ids > 0).long()


def pad_to_multiple(ids, mask, multiple=32):
    """Zero columns (padding id 0, mask 0) appended to ``ids`` / ``mask`` [N, L] up to the next
    multiple of ``multiple``: the bf16 attention kernels take S % 32 == 0, and the added keys are
    masked like any other padding.  A width that is a multiple already comes back unchanged."""
    ids, mask = torch.as_tensor(ids), torch.as_tensor(mask)
    extra = -ids.shape[1] % multiple
    if extra == 0:
        return ids, mask
    return (torch.cat([ids, ids.new_zeros(ids.shape[0], extra)], 1),
            torch.cat([mask, mask.new_zeros(mask.shape[0], extra)], 1))


def train_val_split(input_ids, labels, masks, random_state=2020, test_size=0.1):
    from sklearn.model_selection import train_test_split
    tr_i, va_i, tr_l, va_l = train_test_split(input_ids, labels, random_state=random_state, test_size=test_size)
    tr_m, va_m, _, _ = train_test_split(masks, labels, random_state=random_state, test_size=test_size)
    return (tr_i, tr_m, tr_l), (va_i, va_m, va_l)


@dataclass
class PackedBatch:
    """A padding-free batch: one row per token instead of a [B, S] rectangle.

    Sequence ``b`` owns rows ``cu[b] .. cu[b+1]``; its segment length is its token count rounded up
    to a multiple of 32 (32 <= length <= 512), the extra rows carrying ``ids = 0`` (masked keys, like
    padded columns).  ``rows`` (= T) is a multiple of ``rows_multiple``; the rows from ``cu[B]`` on
    belong to no sequence (``ids = 0``, position 0).  ``max_s`` is the width of the batch the
    sequences came from, rounded up to 32: an upper bound of every segment, the same for every batch
    of a dataset (the attention dropout index is built on it).  ``tokens`` counts the valid tokens."""
    ids: torch.Tensor     # [T] int64
    cu: torch.Tensor      # [B + 1] int32
    pos: torch.Tensor     # [T] int64, 0.. within each segment
    B: int
    max_s: int
    tokens: int
    rows: int

    @property
    def device(self):
        return self.ids.device

    def to(self, device, non_blocking=True):
        return replace(self, ids=self.ids.to(device, non_blocking=non_blocking),
                       cu=self.cu.to(device, non_blocking=non_blocking),
                       pos=self.pos.to(device, non_blocking=non_blocking))

    def unpack(self):
        """-> ids [B, max_s]: the padded rectangle (0 outside the segments)."""
        cu = self.cu.long().cpu()
        out = torch.zeros(self.B, self.max_s, dtype=self.ids.dtype)
        ids = self.ids.cpu()
        for b in range(self.B):
            n = int(cu[b + 1] - cu[b])
            out[b, :n] = ids[cu[b]:cu[b + 1]]
        return out


def pack_batch(ids, mask, multiple=32, rows_multiple=1024) -> PackedBatch:
    """Pack the host batch ``ids`` / ``mask`` [B, W] (see :class:`PackedBatch`).  A sequence's length is
    its last valid mask position + 1; a mask with a hole, or a valid position whose id is 0 (the
    packed key mask is ``ids > 0``), is outside the packed contract and raises.  A sequence without a
    valid position keeps one segment of ``multiple`` masked rows.  Everything here is host data: the
    result is moved with non-blocking copies and nothing waits for the device."""
    ids, mask = torch.as_tensor(ids).long().cpu(), torch.as_tensor(mask).cpu()
    if ids.dim() != 2 or ids.shape != mask.shape:
        raise ValueError(f"pack_batch: ids / mask must be [B, W] of one shape, got {tuple(ids.shape)} / {tuple(mask.shape)}")
    if multiple % 32 or rows_multiple % multiple:
        raise ValueError("pack_batch: multiple must be a multiple of 32 and divide rows_multiple")
    B, W = ids.shape
    valid = mask > 0
    count = valid.sum(1)
    last = W - valid.flip(1).long().argmax(1)            # last valid position + 1 (W when none is valid)
    lens = torch.where(count > 0, last, torch.zeros_like(last))
    if bool((count != lens).any()):
        raise ValueError("pack_batch: a mask with holes is outside the packed contract")
    if bool((ids[valid] <= 0).any()):
        raise ValueError("pack_batch: a valid position with id <= 0 is outside the packed contract")
    max_s = -(-W // 32) * 32
    seg = (lens.clamp_min(1) + multiple - 1) // multiple * multiple
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = seg.cumsum(0)
    used = int(cu[-1])
    rows = max(1, -(-used // rows_multiple)) * rows_multiple
    owner = torch.repeat_interleave(torch.arange(B), seg)
    pos_used = torch.arange(used) - cu[owner]
    pids = torch.zeros(rows, dtype=torch.int64)
    inside = pos_used < lens[owner]
    pids[:used] = torch.where(inside, ids[owner, pos_used.clamp_max(W - 1)], torch.zeros_like(pos_used))
    pos = torch.zeros(rows, dtype=torch.int64)
    pos[:used] = pos_used
    pb = PackedBatch(pids, cu.to(torch.int32), pos, B, max_s, int(count.sum()), rows)
    # the native ops cannot check cu's values without a synchronisation: they are checked here
    assert int(seg.min()) >= 32 and int(seg.max()) <= min(512, max_s) and not bool((seg % 32).any())
    assert rows % rows_multiple == 0 and rows % 32 == 0 and used <= rows and int(pos.max()) < max_s
    return pb


def _pack_args(pack):
    """``pack=`` of the datasets: falsy (padded batches), True (the defaults) or (multiple, rows_multiple)."""
    if not pack:
        return None
    return (32, 1024) if pack is True else (int(pack[0]), int(pack[1]))


class TensorTextDataset:
    """(ids, mask, labels) tensors; ``get_batch`` gathers rows onto the device.  With ``pack`` (True or
    (multiple, rows_multiple)) a batch is ``(PackedBatch, None, labels)`` and ``pack_stats`` sums the
    packed rows, valid tokens and padded rows (B x width) of the batches drawn in epoch 0."""

    def __init__(self, ids, mask, labels, pack=None):
        self.ids = torch.as_tensor(ids, dtype=torch.long)
        self.mask = torch.as_tensor(mask, dtype=torch.long)
        self.labels = torch.as_tensor(labels, dtype=torch.long)
        self.pack = _pack_args(pack)
        self.pack_stats = {"rows": 0, "tokens": 0, "padded_rows": 0}
        self._epoch = 0

    def __len__(self):
        return self.ids.shape[0]

    def set_epoch(self, e):
        self._epoch = e

    def get_batch(self, idx, device=None):
        idx = torch.as_tensor(idx, dtype=torch.long)
        if self.pack:
            pb = pack_batch(self.ids[idx], self.mask[idx], *self.pack)
            if self._epoch == 0:
                self.pack_stats["rows"] += pb.rows
                self.pack_stats["tokens"] += pb.tokens
                self.pack_stats["padded_rows"] += pb.B * pb.max_s
            labels = self.labels[idx]
            if device is not None:
                pb, labels = pb.to(device), labels.to(device, non_blocking=True)
            return pb, None, labels
        out = (self.ids[idx], self.mask[idx], self.labels[idx])
        if device is not None:
            out = tuple(t.to(device, non_blocking=True) for t in out)
        return out
