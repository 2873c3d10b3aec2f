"""The inputs of test_gpu_bytes.py on the CPU: the native oracle (ops.cpu_count)
equals the pure-Python reference (byte_cases.py py_table) on words, counts and
first offsets for every generator and seed the GPU tests use, at bases below,
across and far above 2^32; and the signature twins of the family list really
share a hot-table signature (if the map's formula changes, the twin lists in
byte_cases.py need new words)."""
import pytest

import byte_cases as bc

ops = pytest.importorskip("cuda_mapreduce_amd.ops")

BASES = (0, 2**32 - 5, 2**40 + 12345)

SMALL_SIZES = (1, 31, 32, 33, 2047, 2048, 2049, 70_001)


@pytest.mark.parametrize("name", sorted(bc.TEXTS))
def test_cpu_oracle_equals_python_table(name):
    text = bc.text(name)
    for base in BASES:
        want = bc.py_table(text, base)
        bc.assert_table(ops.cpu_count(text, base), want)
        assert want == bc.table(name, base)  # the shared, shifted copy the GPU tests compare with


def test_cpu_oracle_small_uniform_texts():
    for n in SMALL_SIZES:
        for base in BASES:
            text = bc.random_bytes_text(n, n, 1 / 8)
            bc.assert_table(ops.cpu_count(text, base), bc.py_table(text, base))


def test_py_table_by_hand():
    text = b"  b\x00 a\r\nb\x00 \xff\t\x0b a b"
    assert bc.py_table(text, 100) == ([b"b\x00", b"a", b"\xff\t\x0b", b"b"], [2, 2, 1, 1], [102, 105, 111, 117])
    assert bc.py_table(b"", 7) == ([], [], [])
    assert bc.py_table(b" \r\n", 7) == ([], [], [])


def test_twins_share_a_signature():
    classes = bc.twin_classes()
    assert len(classes) == 8 + 7
    for cls in classes:
        assert len(set(cls)) == len(cls) == bc.TWIN_CLASS
        assert len({len(w) for w in cls}) == 1
        assert len({bc.hot_sig(w) for w in cls}) == 1
    for L in bc.TWIN_LENGTHS:
        a, b = bc.byte7_twins(L)[5], bc.byte7_twins(L)[40]
        assert [i for i in range(L) if a[i] != b[i]] == [7]
        if L >= 9:
            a, b = bc.xor_twins(L)[5], bc.xor_twins(L)[40]
            assert a[0] != b[0] and a[0] ^ a[8] == b[0] ^ b[8] and a[1:8] == b[1:8] and a[9:] == b[9:]
    # some twins can enter the hot table (first 8 bytes' top byte >= 8) and some cannot
    assert {w[7] < 8 for w in bc.byte7_twins(8)} == {True, False}
    # the issue's own example pair
    assert bc.hot_sig(b"abcdefghx") == bc.hot_sig(b"xbcdefgha") != bc.hot_sig(b"abcdefghy")


def test_family_list_covers_the_edges():
    for both in (False, True):
        fam = dict(bc.family_words(both))
        for L in bc.FAMILY_LENGTHS:
            assert b"\x00" * L in fam and b"\xff" * L in fam
            assert sum(1 for w in fam if len(w) == L and w[-1] == 0) >= (2 if L > 1 else 1)
        for c in bc.EDGE_BYTES:
            assert bytes([c]) in fam and b"a" + bytes([c]) + b"b" in fam
        for k in (9, 10, 11, 12):
            assert b"rec16nul" + b"\x00" * (k - 8) in fam
        hot = sum(fam.values())
        assert 0 < hot < len(fam)
        for cls in bc.twin_classes():
            marks = {fam[w] for w in cls}
            assert marks == ({True} if both else {True, False})
