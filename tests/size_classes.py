"""The frame sizes of the size sweep (tests/test_size_sweep_gpu.py, tests/test_cnn_bwd_gpu.py) and the classes they cover.

CamLocDataset(augment=True) hands the network ceil(480 s) x ceil(720 s) frames for s in [2/3, 3/2]: any height in 320...720 and any
width in 480...1080.  What a kernel does at a frame's edges depends on residues of its size only:
  * (H mod 8, W mod 8): whether each of the three stride-2 layers rounds up, which taps of its last row / column fall on padding,
    and - with it - the parity of the map at every level of the stem;
  * (o(H) mod 6, o(W) mod 6) and (o(H) mod 4, o(W) mod 4), o = the cell grid after three ceil-halvings: the partial tiles of
    F(6x6,3x3) and F(4x4,3x3).
SIZES visits every class of all three kinds with 64 small frames; tests/test_size_classes.py pins the counts."""

SIZES = [(40 + a + 8 * ((a + b) % 6), 56 + b + 8 * ((a + 2 * b) % 6)) for a in range(8) for b in range(8)]

# one frame per value of a, b = (3 a + 1) mod 8: H and W of opposite parity, every value of H mod 8 and of W mod 8 once
MIXED_PARITY = [SIZES[8 * a + (3 * a + 1) % 8] for a in range(8)]


def o(n):
    """Three stride-2 3x3 pad-1 convolutions: ceil division each time."""
    for _ in range(3):
        n = (n + 1) // 2
    return n


def ids(sizes):
    return ["%dx%d" % s for s in sizes]
