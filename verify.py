#!/usr/bin/env python3
"""Check a dataset's frames against their recorded poses: every frame's depth map against the render at its joint angles and
camera pose, on the GPU (the reference's Verifier shows the same comparison as pictures and leaves the decision to a person).
Prints the agreement table's summary and the frames whose pose is to be questioned; -sheets writes their overlays as contact
sheets, -remove writes the set without them.  `dataset` may be a 'synthetic:<frames>[:<seed>[:<intrinsics preset>]]' or 'photo:...' name."""
import argparse
import json

import numpy as np

from robotpose import Verifier


def verify(args):
    if args.remove and args.dataset.startswith(('synthetic:', 'photo:')):
        raise SystemExit("-remove: a synthetic set is rendered as it is read and stored nowhere, so there is nothing to rewrite")
    ver = Verifier(args.dataset, batch=args.batch, tol=args.tol)
    table = ver.run()
    flagged, unrendered = ver.flagged(), ver.unrendered()
    print(ver.summary())
    if args.json:
        cells = lambda v: np.where(np.isnan(v), None, v.astype(object)).tolist() if v.dtype.kind == 'f' else v.tolist()      # noqa: E731
        rows = {k: cells(v) for k, v in table.items() if k != 'links'}
        rows['links'] = {k: cells(v) for k, v in table['links'].items()}
        with open(args.json, 'w') as f:
            json.dump({'dataset': args.dataset, 'tol': ver.tol, 'flagged': flagged.tolist(), 'unrendered': unrendered.tolist(),
                       'sums': ver.sums.tolist(), 'table': rows}, f)
        print(f"table in {args.json}")
    if args.sheets and len(flagged):
        paths = ver.sheets(args.sheets, flagged)
        print(f"{len(paths)} contact sheets of the flagged frames in {args.sheets}")
    if args.remove and len(flagged):
        print(f"{len(flagged)} frames removed: the set without them is in {ver.remove(flagged)}")
    return flagged


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', type=str, help="The dataset to verify. Can be a partial name.")
    parser.add_argument('-batch', type=int, default=64, help="Frames per device batch.")
    parser.add_argument('-tol', type=float, default=2 ** -5, help="Metres within which a recorded depth agrees with the render.")
    parser.add_argument('-sheets', type=str, default=None, help="Folder for contact sheets of the flagged frames' overlays.")
    parser.add_argument('-remove', action="store_true", help="Write the set without the flagged frames (as <dataset>_verified).")
    parser.add_argument('-json', type=str, default=None, help="File for the per-frame table.")
    verify(parser.parse_args())
