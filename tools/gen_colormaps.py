"""Writes ppea-depth_amd/ppeadepth/colormaps.json: the 256 x 3 uint8 tables vis.py and ops.colorize look colours up in.

They are matplotlib's listed colormaps as `Colormap.__call__(bytes=True)` returns them: `(colors * 255).astype(uint8)`, the
truncation matplotlib applies to its float table.  Run once per matplotlib release that changes a table (none has since
2.0); the package itself never imports matplotlib.

    python tools/gen_colormaps.py
"""
import json
import os

import numpy as np

NAMES = ("plasma", "magma", "viridis", "inferno")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppea-depth_amd", "ppeadepth",
                   "colormaps.json")


def tables():
    import matplotlib
    out = {}
    for name in NAMES:
        c = np.asarray(matplotlib.colormaps[name].colors, dtype=np.float64)
        assert c.shape == (256, 3), (name, c.shape)
        out[name] = (c * 255).astype(np.uint8)
    return out


if __name__ == "__main__":
    t = tables()
    # text, so that the tables can be read in a diff: per colormap 16 strings of 16 "rrggbb" rows each
    doc = {name: [" ".join(bytes(r).hex() for r in tab[i:i + 16]) for i in range(0, 256, 16)] for name, tab in t.items()}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{OUT}: {', '.join(t)} ({os.path.getsize(OUT)} bytes)")
