#!/usr/bin/env python3
"""Times rope_seg_mask_overlaps (csrc/rope_eval.hip) against the plain torch formulations of the same counts on the same tensors:
8 frames x 7 instances and 8 x 100, at 640x480 and at 160x90.  Per shape: time per call (device events around `reps` calls on
one stream), the bytes a call must read (instance planes plus label planes) and the resulting GB/s; then the torch formulations a
user has without the kernel — boolean planes AND the eight unpacked label planes, summed; and the same as a float32 matmul per
frame — with the label planes unpacked outside the timed region.  Every formulation's counts are compared before anything is timed.
Usage: python tools/bench_seg_eval.py [--reps 200] [--out profiles/seg_eval.txt]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))


def timed(fn, reps, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps                              # ms per call


def main():
    import ctypes as C
    import torch
    from rope_s3d_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    lib = eng.load_library()
    lines = [f"rope_seg_mask_overlaps against torch, {torch.cuda.get_device_name(0)}, build {lib.rope_build_id().decode()}, "
             f"{args.reps} calls per figure (device events; a call = 3 memsets + 2 kernels)",
             f"{'shape':<22}{'MB read':>9}{'kernel ms':>11}{'GB/s':>8}{'and+sum ms':>12}{'matmul ms':>11}{'torch/kernel':>14}"]
    for (H, W) in ((480, 640), (90, 160)):
        for per_frame in (7, 100):
            F = 8
            K = F * per_frame
            g = torch.Generator(device='cuda').manual_seed(H + per_frame)
            masks = torch.rand((K, H, W), device='cuda', generator=g) < 0.2
            gt = torch.randint(0, 256, (F, H, W), device='cuda', generator=g, dtype=torch.uint8)
            first = np.arange(F + 1, dtype=np.int32) * per_frame
            inter, area_pred, area_gt = (torch.empty(s, dtype=torch.int32, device='cuda') for s in ((K, 8), (K,), (F, 8)))
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            p = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731

            def kernel():
                rc = lib.rope_seg_mask_overlaps(p(masks), first.ctypes.data_as(C.c_void_p), F, p(gt), H, W, p(inter), p(area_pred), p(area_gt), stream)
                assert rc == 0, rc

            labels = ((gt[:, None] >> torch.arange(8, device='cuda', dtype=torch.uint8)[None, :, None, None]) & 1).bool()      # (F, 8, H, W)
            labels_f = labels.reshape(F, 8, H * W).float()

            def and_sum():
                m = masks.view(F, per_frame, 1, H, W)
                return (m & labels[:, None]).sum(dim=(3, 4)), masks.sum(dim=(1, 2))

            def matmul():
                m = masks.view(F, per_frame, H * W).float()
                return torch.bmm(m, labels_f.transpose(1, 2)), m.sum(dim=2)

            kernel()
            torch.cuda.synchronize()
            want_i, want_a = and_sum()
            mm_i, mm_a = matmul()
            assert torch.equal(inter.view(F, per_frame, 8).long(), want_i.long()) and torch.equal(area_pred.long(), want_a.long())
            assert torch.equal(mm_i.long(), want_i.long()) and torch.equal(mm_a.reshape(-1).long(), want_a.long())
            assert torch.equal(area_gt.long(), labels.sum(dim=(2, 3)).long())
            reps = args.reps if per_frame == 7 or H < 480 else max(20, args.reps // 4)
            t_k, t_a, t_m = timed(kernel, args.reps), timed(and_sum, reps), timed(matmul, reps)
            nbytes = (K + F) * H * W
            lines.append(f"{f'{F} x {per_frame} @ {W}x{H}':<22}{nbytes / 1e6:>9.2f}{t_k:>11.4f}{nbytes / t_k / 1e6:>8.0f}{t_a:>12.4f}{t_m:>11.4f}"
                         f"{min(t_a, t_m) / t_k:>14.1f}")
            del labels, labels_f, masks, gt
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
