"""gs_render_distortion_backward of ONE build of the library on the eight scenes of tests/render_ref64.py, kept for or
compared with another build's: the record that a restructuring of k_render_distortion_bwd leaves its results alone.

    GSPLAT_HIP_LIB=<the other build's libgsplat_hip.so> python scripts/distortion_bwd_ab.py --save before.pt
    python scripts/distortion_bwd_ab.py --check before.pt [--out profiles/r17/distortion_bwd_bits.json]

Every scene goes through tests/test_gpu_distortion.py's kernel_run with all three incoming gradients (the scene's
grad_image, as the test passes it).  --check holds this build's g_z and slab columns to the saved ones by that test
file's own rules:

    one tile        every address receives exactly one atomic: torch.equal
    several tiles   the sums of a row arrive in another order: noise_measure <= (tiles - 1) x 2^-24 per tensor, over the
                    reference's magnitudes (tests/distortion_ref.py)

Prints one line per scene, writes the record and exits 1 if a scene misses its rule.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", default="")
    ap.add_argument("--check", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from gaussian_splatting_amd import _hip
    from tests import depth_alpha_ref as D
    from tests import distortion_ref as X
    from tests.test_gpu_distortion import SCENES, kernel_run

    fields = X.KEYS + ("distortion", "depth", "alpha", "t_end")
    got = {}
    for name in SCENES:
        gi = X.reference(name).grad_image.float()
        run = kernel_run(D.depth_scene(name), (gi[..., 0], gi[..., 1], gi[..., 2]))
        got[name] = {k: run[k] for k in fields}
    if args.save:
        torch.save(got, args.save)
    if not args.check:
        return 0
    before = torch.load(args.check)
    record = {"what": "gs_render_distortion_backward with (g_dist, g_depth, g_alpha), this build against the saved one",
              "lib": os.path.basename(_hip.LIB_PATH), "scenes": {}}
    ok = True
    for name in SCENES:
        sc, ref = D.depth_scene(name), X.reference(name)
        tiles = sc.ranges.numel() - 1
        row = {"tiles": tiles, "chunks": (int((sc.ranges[1:] - sc.ranges[:-1]).max()) + 63) // 64,
               "forward_equal": all(torch.equal(got[name][k], before[name][k]) for k in fields[len(X.KEYS):]),
               "nonzero": all(bool(got[name][k].any()) for k in X.KEYS)}
        if tiles == 1:
            row["rule"] = "torch.equal"
            row["equal"] = {k: bool(torch.equal(got[name][k], before[name][k])) for k in X.KEYS}
            row["pass"] = all(row["equal"].values())
        else:
            row["rule"] = "noise_measure <= (tiles - 1) * 2^-24"
            row["bound"] = (tiles - 1) * 2.0 ** -24
            row["noise_measure"] = {k: X.noise_measure(got[name][k], before[name][k], ref.abs[k]) for k in X.KEYS}
            row["equal"] = {k: bool(torch.equal(got[name][k], before[name][k])) for k in X.KEYS}
            row["pass"] = all(m <= row["bound"] for m in row["noise_measure"].values())
        row["pass"] = row["pass"] and row["forward_equal"] and row["nonzero"]
        ok = ok and row["pass"]
        record["scenes"][name] = row
        print(json.dumps({name: row}), flush=True)
    record["all_pass"] = ok
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
