"""Inputs over all 256 byte values and the key-class edges, and an independent
reference table for them (helper module of test_byte_inputs_cpu.py,
test_gpu_bytes.py and test_gpu_props.py).

The reference, py_table, is written from the semantics alone: delimiters are
exactly {0x20, 0x0D, 0x0A}, every other byte (NUL, TAB, 0x80..0xFF) is a word
byte, words are listed in first-occurrence order with their count and the
offset of their first byte, a last word without a delimiter counts.  It knows
nothing of the key scheme.

The generators do know it (docs/DESIGN.md "Keys"): they aim words at the edges
of the key classes (lengths 7/8, 8/9, 12/13, 15/16, 64/65) and at the two
encodings that are valid only for some words — the 16-byte record without a
length (last byte nonzero, bytes [8, len) not all zero) and the hot table's
two-word signature, which many words share (hot_sig below; the map tells them
apart by the side word alone)."""
import functools
import re

import numpy as np

DELIMS = (0x20, 0x0D, 0x0A)
_WORD = re.compile(rb"[^\x20\x0d\x0a]+")


def py_table(text, base=0):
    """(words, counts, first offsets) of `text` placed at offset `base`."""
    index, words, counts, first = {}, [], [], []
    for m in _WORD.finditer(bytes(text)):
        w = m.group()
        i = index.get(w)
        if i is None:
            index[w] = len(words)
            words.append(w)
            counts.append(1)
            first.append(base + m.start())
        else:
            counts[i] += 1
    return words, counts, first


def assert_table(got, want):
    """A Result equals a py_table triple: words, order, counts, first offsets, total."""
    words, counts, first = want
    assert got.total == sum(counts)
    assert len(got.words) == len(words)
    assert got.words == words
    assert np.array_equal(got.counts, np.array(counts, np.uint64))
    assert np.array_equal(got.first_off, np.array(first, np.uint64))


# ------------------------------------------------------------------ families --
FAMILY_LENGTHS = tuple(range(1, 18)) + (24, 31, 32, 33, 63, 64, 65)
EDGE_BYTES = (0x00, 0x09, 0x0B, 0x0C, 0x0E, 0x1F, 0x21, 0x7F, 0x80, 0x8A, 0x8D, 0xA0, 0xFF)
TWIN_LENGTHS = tuple(range(8, 16))
TWIN_CLASS = 64  # words per signature class (the issue asks for two; more make shared groups likely)
LOW7 = (1 << 56) - 1


def hot_sig(word):
    """The map's hot-table signature of an 8..15-byte word (map.hip inline_key):
    low 7 bytes of (first 8 bytes ^ bytes [8, len)), the length on top."""
    assert 8 <= len(word) <= 15
    k0 = int.from_bytes(word[:8], "little")
    t = int.from_bytes(word[8:], "little")
    return ((t ^ k0) & LOW7) | (len(word) << 56)


def _base(L):
    # distinct per length, bytes 0x30..0x7E: no delimiter, last byte neither 0x00 nor 0xFF
    return bytes(0x30 + ((3 * i + 5 * L) % 0x4F) for i in range(L))


def _word_bytes():
    return [c for c in range(256) if c not in DELIMS]


def _spread(vals):
    # TWIN_CLASS of them, evenly spaced, both ends included
    return [vals[i * (len(vals) - 1) // (TWIN_CLASS - 1)] for i in range(TWIN_CLASS)]


def byte7_twins(L):
    """TWIN_CLASS words of length L that differ only in byte index 7 (byte 7
    spread over 0x00..0xFF: values below 8 keep a word out of the hot table)."""
    stem = bytearray(b"Tw" + bytes([0x40 + L]) + _base(L)[3:])
    vals = _spread(_word_bytes())
    out = []
    for v in vals:
        w = bytearray(stem)
        w[7] = v
        out.append(bytes(w))
    return out


def xor_twins(L):
    """TWIN_CLASS words of length L >= 9 with bytes 1..7 and 9.. equal and one
    value of byte 0 ^ byte 8: pairs such as abcdefgh+x / xbcdefgh+a."""
    stem = bytearray(b"?x" + bytes([0x50 + L]) + _base(L)[3:])
    c = 0x19  # 'a' ^ 'x'
    vals = [v for v in _word_bytes() if (v ^ c) not in DELIMS]
    vals = _spread(vals)
    out = []
    for v in vals:
        w = bytearray(stem)
        w[0], w[8] = v, v ^ c
        out.append(bytes(w))
    return out


def twin_classes():
    """Every signature class of the family list: lists of words sharing one hot_sig."""
    return [byte7_twins(L) for L in TWIN_LENGTHS] + [xor_twins(L) for L in TWIN_LENGTHS if L >= 9]


def family_words(both_twins_hot=False):
    """[(word, hot)] — the fixed family list, duplicates removed (first mark kept)."""
    fam = []
    for L in FAMILY_LENGTHS:
        b = _base(L)
        for v, w in enumerate((b, b[:-1] + b"\x00", b[:-1] + b"\xff", b"\x00" * L, b"\xff" * L)):
            fam.append((w, (L + v) % 2 == 0))
    for cls in twin_classes():
        for i, w in enumerate(cls):
            fam.append((w, both_twins_hot or i % 2 == 0))
    # 16-byte record edges: a tail of NULs only, and the 12/13 and 8/9 length steps
    for k in range(1, 5):
        fam.append((b"rec16nul" + b"\x00" * k, k % 2 == 1))
    fam += [(b"twelve_bytes", True), (b"twelve_bytesQ", False), (b"octoword", False), (b"octowordZ", True)]
    # the neighbours of the three delimiters, and both ends of the byte range
    for i, c in enumerate(EDGE_BYTES):
        fam.append((bytes([c]), i % 2 == 0))
        fam.append((b"a" + bytes([c]) + b"b", i % 2 == 1))
    # exact / hashed keys, and the longest LONG word the hot table holds
    q15, r64 = b"fifteen_bytes_x", b"sixty-four:" + _base(64)[11:]
    fam += [(q15, True), (q15 + b"!", False), (r64, True), (r64 + b"~", True)]
    seen, out = set(), []
    for w, hot in fam:
        assert w and not any(c in DELIMS for c in w)
        if w not in seen:
            seen.add(w)
            out.append((w, hot))
    return out


SEPS = (b" ", b"\n", b"\r\n", b"  ")


def family_text(seed, n_words, hot_share=0.9, both_twins_hot=False):
    """n_words draws from family_words(): hot_share of them from the hot subset
    (frequent enough for the sampled hot table), the rest spread over the cold
    words (a handful of occurrences each: they travel as records)."""
    fam = family_words(both_twins_hot)
    hot = [w for w, h in fam if h]
    cold = [w for w, h in fam if not h]
    rng = np.random.default_rng(seed)
    is_hot = rng.random(n_words) < hot_share
    hi = rng.integers(0, len(hot), n_words)
    ci = rng.integers(0, max(len(cold), 1), n_words)
    si = rng.integers(0, len(SEPS), n_words)
    out = []
    for i in range(n_words):
        out.append(hot[hi[i]] if is_hot[i] or not cold else cold[ci[i]])
        out.append(SEPS[si[i]])
    return b"".join(out)


# ---------------------------------------------------------------- LONG tails --
LONG_TAIL_LENGTHS = (16, 17, 23, 24, 25, 56, 57, 63, 64, 65, 66)


def long_tail_words(seed):
    """Per length 40 LONG words sharing their first 8 bytes: 20 share all but
    the last byte, 20 have tails of arbitrary word bytes."""
    rng = np.random.default_rng(seed)
    wb = np.array(_word_bytes(), np.uint8)
    words = []
    for L in LONG_TAIL_LENGTHS:
        prefix = b"LT%02d_pfx" % L
        assert len(prefix) == 8
        stem = prefix + bytes(wb[rng.integers(0, len(wb), L - 9)])
        lasts = rng.choice(wb, 20, replace=False)
        group = {stem + bytes([c]) for c in lasts}
        while len(group) < 40:
            group.add(prefix + bytes(wb[rng.integers(0, len(wb), L - 8)]))
        words += sorted(group)
    return words


def long_tail_text(seed, n_words=40000):
    """60 % LONG words of long_tail_words (Zipf-weighted: the head is hot, the
    tail occurs once or twice), 40 % short and medium words."""
    rng = np.random.default_rng(seed)
    longs = long_tail_words(seed)
    order = rng.permutation(len(longs))
    other = [b"a", b"bb", b"ccccccccc", b"medium_word_15b", b"LT16_pfx", b"LT64_pfxyz", b"\xff\x00", b"\x00"]
    pick_long = rng.random(n_words) < 0.6
    z = rng.zipf(1.2, n_words)
    oi = rng.integers(0, len(other), n_words)
    si = rng.integers(0, len(SEPS), n_words)
    out = []
    for i in range(n_words):
        out.append(longs[order[int(z[i]) % len(longs)]] if pick_long[i] else other[oi[i]])
        out.append(SEPS[si[i]])
    return b"".join(out)


# ------------------------------------------------------------- uniform bytes --
def random_bytes_text(seed, n, p_delim):
    """n bytes uniform over 0..255, a fraction p_delim of the positions
    overwritten by a random delimiter."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    d = rng.random(n) < p_delim
    a[d] = np.array(DELIMS, np.uint8)[rng.integers(0, 3, int(d.sum()))]
    return a.tobytes()


# ------------------------------------------------- the texts the tests share --
def _synthetic():
    from cuda_mapreduce_amd import ops

    return ops.synth_host(SYNTH["nbytes"], seed=SYNTH["seed"], vocab=SYNTH["vocab"])


SYNTH = dict(nbytes=4 << 20, seed=17, vocab=60000)  # also generated on the device (Engine.synth_device)
TEXTS = {
    "family-one-hot": lambda: family_text(1, 200_000),
    "family-both-hot": lambda: family_text(2, 200_000, both_twins_hot=True),
    "long-tail": lambda: long_tail_text(3),
    "uniform-1/3": lambda: random_bytes_text(11, 2 << 20, 1 / 3),
    "uniform-1/8": lambda: random_bytes_text(12, 2 << 20, 1 / 8),
    "uniform-1/40": lambda: random_bytes_text(13, 2 << 20, 1 / 40),
    "synthetic": _synthetic,
}


@functools.lru_cache(maxsize=None)
def text(name):
    return TEXTS[name]()


@functools.lru_cache(maxsize=None)
def _table0(name):
    return py_table(text(name))


def table(name, base=0):
    """py_table(text(name), base), the scan done once per text."""
    words, counts, first = _table0(name)
    return words, counts, [base + f for f in first]
