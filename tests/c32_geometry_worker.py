"""Worker of tests/test_gpu_c32_geometry.py: one configuration of the CG preconditioner with the launch regime of its
polynomial steps pinned by TLFEA_C32_REGIME (the library reads its switches once per process; the caller sets the
environment).  The operator checks are those of tests/precond_worker.py, run unchanged; around them this worker reads the
geometry hook after every preconditioner application and after the solve, and FAILS when the pinned regime did not run on
the levels the configuration names, or when a level lacks a precondition the configuration asks for.

    python tests/c32_geometry_worker.py '<json config>' <out.npz>

config: name, problem, opts, expect (handed on to precond_worker), and
  pin      {level: [regime, lanes, upfront]}: what the hook must report for that level (0 fine, 1 vertex, 2 third)
  need     {precondition: level}: the level that must show it, in its pinned geometry --
           long  a row with more blocks than lanes x up-front slots (the further-rounds loop)
           short a row with fewer blocks than lanes (masked lanes in the first slot)
           tail  a row count that is no multiple of the rows per workgroup (masked tail group)
           small fewer rows than one workgroup holds
Prints precond_worker's JSON line extended by geometry, levels and sha256 of the block application's result."""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import precond_worker as pw  # noqa: E402

SEEN = dict(geometry=[], levels={}, sha=None)


class Probe(pw.tl.SyncedNewtonSolver):
    def _note(self):
        SEEN["geometry"].append([self.GetC32Geometry(level) for level in range(3)])

    def ApplyPreconditioner(self, r):
        z = super().ApplyPreconditioner(r)
        self._note()
        if np.ndim(r) == 2:
            SEEN["sha"] = hashlib.sha256(np.ascontiguousarray(z).tobytes()).hexdigest()
        return z

    def LinearSolve(self, b):
        out = super().LinearSolve(b)
        self._note()
        return out

    def RetrieveHessianCSRToCPU(self):
        ro, ci, val = super().RetrieveHessianCSRToCPU()
        SEEN["levels"][0] = np.diff(ro)[::3] // 3
        return ro, ci, val

    def RetrievePmgLevel(self):
        out = super().RetrievePmgLevel()
        SEEN["levels"][1] = np.diff(out[2])
        return out

    def RetrievePmgLevel3(self):
        out = super().RetrievePmgLevel3()
        SEEN["levels"][2] = np.diff(out[3])
        return out


def main(cfg, out_path):
    pw.tl.SyncedNewtonSolver = Probe
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        pw.main(dict(name=cfg["name"], problem=cfg["problem"], opts=cfg["opts"], expect=cfg.get("expect", {})), out_path)
    out = json.loads(buf.getvalue().strip().splitlines()[-1])
    levels = {str(k): dict(rows=int(len(b)), blocks_min=int(b.min()), blocks_max=int(b.max())) for k, b in SEEN["levels"].items()}
    out.update(geometry=SEEN["geometry"], level_sizes=levels, sha=SEEN["sha"])
    print(json.dumps(out), flush=True)   # the facts first: a failed assertion below is then read against them
    assert len(SEEN["geometry"]) >= 5, "the hook was not read after every application and the solve"
    for level, (regime, lanes, upfront) in cfg["pin"].items():
        for geo in SEEN["geometry"]:     # every application and the solve took the pinned path on this level
            g = geo[int(level)]
            assert (g["regime"], g["lanes"], g["upfront"]) == (regime, lanes, upfront), (cfg["name"], "level", level, g)
            if regime == 3:              # one round: every workgroup resident at once, by the occupancy query itself
                assert 1 <= g["grid"] <= g["resident"], (cfg["name"], "level", level, g)
    for what, level in cfg.get("need", {}).items():
        assert str(level) in cfg["pin"], (cfg["name"], what, "names a level that is not pinned")
        g, lv = SEEN["geometry"][-1][int(level)], levels[str(level)]
        per_wg = g["rows_per_group"] * (g["threads"] // g["lanes"])
        ok = dict(long=lv["blocks_max"] > g["lanes"] * g["upfront"], short=lv["blocks_min"] < g["lanes"],
                  tail=lv["rows"] % per_wg != 0, small=lv["rows"] < per_wg)[what]
        assert ok, (cfg["name"], what, "does not hold on level", level, lv, g)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
