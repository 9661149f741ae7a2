"""Generates tests/golden/rtrans_slices_phong.npz: the rough-transmittance slices and Fdr of the rough-plastic surfaces that carry
the Phong microfacet distribution (GVPM_MICROFACET_PHONG), reduced from the reference's data/microfacet/phong.dat exactly as
make_rtrans_golden.py reduces beckmann.dat and ggx.dat (its reader and its two reductions, imported).  Same keys, same layout:
100 values + Fdr per surface."""
import os

import numpy as np

from make_rtrans_golden import DATA_DIR, F, key, read_dat, reduce_slice

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rtrans_slices_phong.npz")
# (eta, alpha): the walls of cbox_roughplastic_phong, and the one-component corner of the relabelled tables
ENTRIES = ((1.5, 0.1), (1.5, 0.3), (1.5, 0.03))


def make():
    table = read_dat(os.path.join(DATA_DIR, "phong.dat"))
    out = {}
    for eta, alpha in ENTRIES:
        sl, fdr = reduce_slice(table, eta, alpha)
        out[key("phong", eta, alpha)] = np.concatenate([sl, [fdr]]).astype(F)
    return out


if __name__ == "__main__":
    np.savez(OUT, **make())
    for k, v in np.load(OUT).items():
        print(k, "T(0) %.4f T(1) %.4f Fdr %.4f" % (v[0], v[99], v[100]))
