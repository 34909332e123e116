"""CPU: the size list of the sweep covers every residue class the kernels' edge handling depends on (tests/size_classes.py).
Whoever edits the list cannot lose a class unnoticed."""
from size_classes import MIXED_PARITY, SIZES, o


def test_the_size_list_is_the_stated_range():
    assert len(SIZES) == len(set(SIZES)) == 64
    assert SIZES[0] == (40, 56) and min(h for h, _ in SIZES) == 40 and min(w for _, w in SIZES) == 56
    assert max(h for h, _ in SIZES) == 87 and max(w for _, w in SIZES) == 103


def test_every_residue_class_of_the_stem_and_of_both_winograd_tilings_is_covered():
    assert len({(h % 8, w % 8) for h, w in SIZES}) == 64
    assert len({(o(h) % 6, o(w) % 6) for h, w in SIZES}) == 36
    assert len({(o(h) % 4, o(w) % 4) for h, w in SIZES}) == 16


def test_all_four_parity_classes_at_every_level_of_the_stem():
    """What (H mod 8, W mod 8) carries: after k ceil-halvings the parities of the map are those of ceil(H / 2^k), ceil(W / 2^k)."""
    for level in range(3):
        seen = set()
        for h, w in SIZES:
            for _ in range(level):
                h, w = (h + 1) // 2, (w + 1) // 2
            seen.add((h % 2, w % 2))
        assert len(seen) == 4, (level, seen)


def test_the_mixed_parity_subset():
    assert len(MIXED_PARITY) == 8 and all(s in SIZES for s in MIXED_PARITY)
    assert all((h + w) % 2 == 1 for h, w in MIXED_PARITY)
    assert {h % 8 for h, _ in MIXED_PARITY} == set(range(8)) == {w % 8 for _, w in MIXED_PARITY}
