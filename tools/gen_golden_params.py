#!/usr/bin/env python3
"""Golden record of the reference's production parameter files as `params.load_param_file` reads them
(data/par/par4rl/production/<name>.py of the reference, for every name of params.BUILTIN_NAMES; run where the
reference tree exists):

    python tools/gen_golden_params.py REFERENCE_ROOT

Writes tests/golden/param_files.json: per file, every attribute of every parameter object after loading (the
settings alone, as data; arrays with their dtype).  tests/test_geometry.py checks the built-in parameter sets
against it and replays it through the loader.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ao_marl_amd import params  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "param_files.json")
GROUPS = ("p_loop", "p_geom", "p_tel", "p_atmos", "p_targets", "p_wfss", "p_dms", "p_centroiders", "p_controllers")


def encode(v):
    if isinstance(v, np.ndarray):
        return {"ndarray": v.tolist(), "dtype": v.dtype.str}
    if isinstance(v, np.generic):
        return {"scalar": v.item(), "dtype": v.dtype.str}
    if isinstance(v, (list, tuple)):
        return [encode(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError("unexpected parameter value %r" % (v,))


def record(ps):
    out = {"simul_name": ps.simul_name}
    for grp in GROUPS:
        g = getattr(ps, grp)
        objs = g if isinstance(g, list) else [g]
        rec = [{"class": type(o).__name__, "attrs": {k: encode(v) for k, v in sorted(vars(o).items())}} for o in objs]
        out[grp] = rec if isinstance(g, list) else rec[0]
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: gen_golden_params.py REFERENCE_ROOT")
    ref = sys.argv[1]
    prod = os.path.join(ref, "data", "par", "par4rl", "production")
    got = {name: record(params.load_param_file(os.path.join(prod, name + ".py"))) for name in params.BUILTIN_NAMES}
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d files)" % (OUT, len(got)))


if __name__ == "__main__":
    main()
