"""The input map of the byte path (tnml_set_input_map, include/tnml.h): geometry of a block-sum reduction plus the table
that turns a block sum into the two local features of a site.  Host arithmetic only -- nothing here touches the GPU."""
import numpy as np

from . import hostlib


class InputMap:
    """src_rows x src_cols raw bytes -> out_rows x out_cols sites; site (r, c) is the SUM of the block x block square whose top-left
    corner is (row0 + block r, col0 + block c), and its features are table[sum]."""

    def __init__(self, src_rows, src_cols, block, row0, col0, out_rows, out_cols, table, feature=None):
        self.src_rows, self.src_cols, self.block = int(src_rows), int(src_cols), int(block)
        self.row0, self.col0 = int(row0), int(col0)
        self.out_rows, self.out_cols = int(out_rows), int(out_cols)
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        self.feature = feature                      # a name for print-outs; None for a table given by the caller
        if self.table.ndim != 2 or self.table.shape[1] != 2:
            raise ValueError("table must have shape [ncodes, 2]")

    @property
    def S(self):
        """bytes per raw image"""
        return self.src_rows * self.src_cols

    @property
    def N(self):
        """sites"""
        return self.out_rows * self.out_cols

    @property
    def ncodes(self):
        return int(self.table.shape[0])

    @classmethod
    def from_imglen(cls, side, imglen, feature="series", scale=1.0):
        """the drivers' `imglen` (mnist_idx.h reduce): bsize = side // imglen, blocks start at side % bsize, for a feature map of the
        drivers (`feature`, `feature_scale`); imglen == side keeps the image (block 1)"""
        side, imglen = int(side), int(imglen)
        if imglen < 1 or imglen > side:
            raise ValueError("reduce: imglen must be between 1 and the image side")
        if imglen == side:
            bsize, rem = 1, 0
        else:
            bsize = side // imglen
            rem = side % bsize
        return cls(side, side, bsize, rem, rem, imglen, imglen, hostlib.feature_table(feature, scale, bsize), feature=feature)

    def with_table(self, table):
        """the same geometry with another table"""
        return InputMap(self.src_rows, self.src_cols, self.block, self.row0, self.col0, self.out_rows, self.out_cols, table)

    def codes(self, pixels):
        """numpy reference of the block sums: pixels[n, S] bytes -> int32 [n, N], sites in row-major order of the reduced image"""
        px = np.asarray(pixels)
        if px.ndim != 2 or px.shape[1] != self.S:
            raise ValueError("pixels must have shape [n, %d], got %s" % (self.S, px.shape))
        img = px.reshape(-1, self.src_rows, self.src_cols).astype(np.int32)
        b = self.block
        win = img[:, self.row0:self.row0 + b * self.out_rows, self.col0:self.col0 + b * self.out_cols]
        if win.shape[1:] != (b * self.out_rows, b * self.out_cols):
            raise ValueError("a block leaves the source image")
        return win.reshape(-1, self.out_rows, b, self.out_cols, b).sum(axis=(2, 4)).reshape(-1, self.N)

    def features(self, pixels):
        """table[codes(pixels)]: phi[n, N, 2], the input of the fp64 feature path for the same images"""
        return self.table[self.codes(pixels)]

    def describe(self):
        """the drivers' `Input map:` line"""
        return "Input map: %d x %d bytes -> %d x %d sites (%d x %d block sums from (%d, %d)), feature = %s, %d codes" % (
            self.src_rows, self.src_cols, self.out_rows, self.out_cols, self.block, self.block, self.row0, self.col0,
            self.feature or "table", self.ncodes)
