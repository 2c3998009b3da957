#!/usr/bin/env python3
"""Mask R-CNN training annotations of a dataset from renders at its recorded poses (same command line as the reference's
annotate.py).  `dataset` may be a 'synthetic:<frames>[:<seed>[:<intrinsics preset>]]' or 'photo:...' name."""
import argparse

from robotpose import AutomaticAnnotator, DatasetRenderer


def label(args):
    rend = DatasetRenderer(args.dataset)
    seg = AutomaticAnnotator(args.dataset, rend, not args.no_preview)
    seg.run()
    print(f"annotations of {seg.ds.length} frames in {seg.dest_path}")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', type=str, help="The dataset to load to annotate. Can be a partial name.")
    parser.add_argument('-no_preview', action="store_true", help="Disables preview.")
    label(parser.parse_args())
