#!/usr/bin/env python3
"""Polish a dataset's recorded camera pose and joint angles against its depth frames in ONE solve, and say how sure the result is.

When many frames of a set disagree with their renders (verify.py), the question is whether the camera pose or an encoder zero is
off.  `-joints offset` answers it: the recorded angles are trusted up to one constant offset per joint, shared by all frames, and
these offsets are solved for together with the six camera parameters (kinematic calibration).  `-joints frame` lets every frame's
angles move on their own beside the camera (bundle polish); `-joints fixed` takes the angles as exact (CameraPoseRefiner).  The
start is the recorded camera pose of the first frame and the recorded angles; the depth frames are down-sampled by -ds_factor as the
camera predictors do.  `dataset` may be a 'synthetic:<frames>[:<seed>[:<intrinsics preset>]]' or 'photo:...' name.

The sigmas are FORMAL (prediction/refinement.py: formal_sigma): they tell what the views pin down and rank, they are no error bars."""
import argparse
import json

import numpy as np


def calibrate(args):
    from rope_s3d_amd.data.dataset import open_dataset
    from rope_s3d_amd.imgproc import resize_linear
    from rope_s3d_amd.prediction.refinement import BundleRefiner, CameraPoseRefiner
    from rope_s3d_amd.simulation.render import Renderer
    ds = open_dataset(args.dataset)
    n = min(int(args.frames), int(ds.length)) if args.frames else int(ds.length)
    if n < 1:
        raise SystemExit("no frames to calibrate on")
    angles = np.asarray(ds.angles[:n], np.float64).reshape(-1, 6)
    pose0 = np.asarray(ds.camera_pose[:n], np.float64).reshape(-1, 6)[0].copy()
    full = np.asarray(ds.depthmaps[:n], np.float32)
    f = int(args.ds_factor)
    h, w = full.shape[1] // f, full.shape[2] // f
    depth = np.stack([resize_linear(d, w, h) for d in full]).astype(np.float32) if f > 1 else full
    mask, extra = None, {}
    if args.silhouette > 0 and args.native:
        raise SystemExit("-native polishes on the depth term alone: it does not go with -silhouette")
    if args.robust and (args.native or args.silhouette > 0 or args.joints == 'fixed'):
        raise SystemExit("-robust weighs the depth term of the host loop: it goes with -joints frame or offset, not with -native or -silhouette")
    if args.both_ways and not args.silhouette > 0:
        raise SystemExit("-both_ways is the second direction of the outline term: it goes with -silhouette")
    if args.robust:
        extra = dict(robust=args.robust, robust_scale='auto' if args.robust_scale is None else args.robust_scale)
    if args.silhouette > 0:
        # the robot masks: the frames' colour images reduced as the depth is, read by the colour code of the set (ColorSegmenter, what
        # Predictor(color_dict=...) sets reads its link masks with); masks made by a segmentation network are not taken here
        if args.joints == 'fixed':
            raise SystemExit("-silhouette goes with -joints frame or offset: -joints fixed is the camera-only polish, which has no such term")
        if not ds.attrs.get('color_dict'):
            raise SystemExit("-silhouette needs a dataset with a color_dict (colour-coded frames): its robot masks are read off the link colours")
        from rope_s3d_amd.segmentation import ColorSegmenter
        from rope_s3d_amd.urdf import URDFReader
        seg = ColorSegmenter(['BG'] + list(URDFReader().mesh_names[:6]), ds.attrs['color_dict'])
        colour = np.asarray(ds.og_img[:n], np.uint8)
        mask = np.zeros((n, h, w), bool)
        for i, c in enumerate(colour):
            m = seg(resize_linear(c, w, h) if f > 1 else c)['masks']
            mask[i] = m.any(axis=2)
        extra = dict(silhouette=args.silhouette, radius=args.radius, both_ways=bool(args.both_ways))
    renderer = Renderer('seg', pose0, str(ds.attrs['color_intrinsics']), intrinsic_ds_factor=f if f > 1 else None)
    try:
        if args.joints == 'fixed' and args.native:
            # the camera alone through rope_refine_bundle: 'frame' mode with no joint refined
            res = BundleRefiner(renderer, renderer.intrinsics, do_angles='', joints='frame', clip=args.clip, iterations=args.iterations,
                                native=True).refine(pose0, angles, depth)
            sigma_pose, out_angles = res.sigma_pose, angles
        elif args.joints == 'fixed':
            res = CameraPoseRefiner(renderer, renderer.intrinsics, clip=args.clip, iterations=args.iterations).refine(pose0, angles, depth)
            sigma_pose, out_angles = res.sigma, angles
        else:
            res = BundleRefiner(renderer, renderer.intrinsics, do_angles=args.do_angles, joints=args.joints, clip=args.clip,
                                iterations=args.iterations, native=args.native, **extra).refine(pose0, angles, depth, mask)
            sigma_pose, out_angles = res.sigma_pose, res.angles
    finally:
        renderer.engine.close()
    worst = np.argsort(-res.frame_cost)[:min(5, n)]
    rep = dict(dataset=args.dataset, frames=n, joints=args.joints, native=bool(args.native), do_angles=args.do_angles, ds_factor=f, clip=args.clip, start_pose=pose0.tolist(),
               pose=res.pose.tolist(), sigma_pose=sigma_pose.tolist(), cost_before=float(res.cost_before), cost_after=float(res.cost_after),
               steps_taken=int(res.steps_taken), inliers=float(res.inliers), frame_cost=res.frame_cost.tolist(), worst_frames=worst.tolist())
    if args.silhouette > 0:
        rep.update(silhouette=args.silhouette, radius=args.radius, cost_silhouette_before=float(res.cost_silhouette_before),
                   cost_silhouette_after=float(res.cost_silhouette_after), inliers_silhouette=float(res.inliers_silhouette),
                   both_ways=bool(args.both_ways), inliers_silhouette_reverse=float(res.inliers_silhouette_reverse))
    if args.robust:
        rep.update(robust=args.robust, robust_scale=float(res.robust_scale))
    names = ('x', 'y', 'z', 'a3', 'a4', 'a5')
    print(f"{args.dataset}: {n} frames at {w} x {h}, joints {args.joints}, {res.steps_taken} steps, {res.inliers:.0f} inlier pixels")
    print(f"mean truncated cost {res.cost_before:.6e} -> {res.cost_after:.6e} m^2" if not args.robust else
          f"mean {args.robust} cost at scale {res.robust_scale:.6f} m {res.cost_before:.6e} -> {res.cost_after:.6e} m^2")
    if args.silhouette > 0:
        print(f"mean truncated outline cost {res.cost_silhouette_before:.6e} -> {res.cost_silhouette_after:.6e} pixels^2 "
              f"(weight {args.silhouette:g}, radius {args.radius}, {res.inliers_silhouette:.0f} contour pixels" +
              (f" of the renders and {res.inliers_silhouette_reverse:.0f} of the masks, both ways)" if args.both_ways else ")"))
    for k in range(6):
        print(f"  {names[k]:>2} {pose0[k]:+.6f} -> {res.pose[k]:+.6f}  (change {res.pose[k] - pose0[k]:+.2e}, formal sigma {sigma_pose[k]:.2e})")
    if args.joints == 'offset':
        rep.update(offsets=res.offsets.tolist(), sigma_offsets=res.sigma_offsets.tolist())
        for j in range(6):
            if not np.isnan(res.sigma_offsets[j]):
                print(f"  zero offset of joint {'SLUBRT'[j]}: {res.offsets[j]:+.6f} rad (formal sigma {res.sigma_offsets[j]:.2e})")
    elif args.joints == 'frame':
        d = out_angles - angles
        rep.update(angle_change_max=np.abs(d).max(axis=0).tolist(), angle_change_rms=np.sqrt((d * d).mean(axis=0)).tolist(),
                   sigma_angles=res.sigma_angles.tolist(), angles=out_angles.tolist())
        for j in range(6):
            if not np.isnan(res.sigma_angles[:, j]).all():
                print(f"  joint {'SLUBRT'[j]}: changed by at most {np.abs(d[:, j]).max():.2e}, RMS {np.sqrt((d[:, j] ** 2).mean()):.2e} rad "
                      f"(median formal sigma {np.median(res.sigma_angles[:, j]):.2e})")
    print("frames with the largest cost: " + ', '.join(f"{i} ({res.frame_cost[i]:.3e})" for i in worst))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(rep, fh)
        print(f"report in {args.json}")
    return rep


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', type=str, help="The dataset to calibrate on. Can be a partial name.")
    parser.add_argument('-frames', type=int, default=0, help="Use the first N frames (0: all).")
    parser.add_argument('-joints', choices=('frame', 'offset', 'fixed'), default='offset',
                        help="frame: every frame's angles are unknowns; offset: one zero offset per joint; fixed: the camera alone.")
    parser.add_argument('-do_angles', type=str, default='SLU', help="The joints to solve for, letters of SLUBRT.")
    parser.add_argument('-ds_factor', type=int, default=4, help="Down-sampling of the frames.")
    parser.add_argument('-iterations', type=int, default=5, help="Rounds at most.")
    parser.add_argument('-clip', type=float, default=2 ** -5, help="Metres at which a residual is truncated.")
    parser.add_argument('-silhouette', type=float, default=0.0,
                        help="Weight of the outline term beside the depth term (0: off). Needs a colour-coded dataset (color_dict).")
    parser.add_argument('-radius', type=int, default=8, help="Pixels at which the outline distance is truncated, 1 .. 16.")
    parser.add_argument('-both_ways', action='store_true',
                        help="With -silhouette: measure the masks' outlines against the render as well as the render's against the masks.")
    parser.add_argument('-robust', choices=('huber', 'tukey'), default=None,
                        help="Weigh the depth residuals (Huber or Tukey) instead of counting them fully up to -clip. Host loop, depth term only.")
    parser.add_argument('-robust_scale', type=float, default=None,
                        help="Scale of the robust weights in metres, at most -clip (default: from the residuals at the start).")
    parser.add_argument('-native', action='store_true',
                        help="Run the loop inside the library (rope_refine_bundle): the solves on the device. Depth term only.")
    parser.add_argument('-json', type=str, default=None, help="File for the report.")
    calibrate(parser.parse_args())
