"""Word sets for the word-order tests (helper module of test_word_order_cpu.py
and test_gpu_word_order.py).

Word order = plain bytewise order, ``sorted()`` on ``bytes``: bytes compare
unsigned, a proper prefix comes first.  The sets aim at what the key scheme
(docs/DESIGN.md "Keys") makes hard: the first 8 bytes of a word are kept
zero-padded, so NUL bytes of a word and padding look alike; bytes 0x80..0xFF
must sort after ASCII; the classes change at 8/9 and 15/16 bytes."""

NUL_LADDER = [b"ab" + b"\0" * j for j in range(21)] + [b"ab\x01"]
NUL_WORDS = [b"\0" * L for L in (1, 8, 9, 15, 16, 17)]
HIGH_BYTES = [b"\x7f", b"\x80", b"\xff", b"\x7fz", b"\x80z", b"\xffz", b"\x7f" * 9, b"\x80" * 9, b"\xff" * 17]
A_CHAIN = [b"a" * L for L in range(1, 41)]


def ladders():
    """The four sets together, distinct words."""
    out = NUL_LADDER + NUL_WORDS + HIGH_BYTES + A_CHAIN
    assert len(set(out)) == len(out)
    return out


def want_perm(words):
    return sorted(range(len(words)), key=words.__getitem__)
