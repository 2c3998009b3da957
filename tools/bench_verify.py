#!/usr/bin/env python3
"""Times rope_frame_agreement (csrc/rope_verify.hip) against a plain torch formulation of the same 28 sums on the same tensors:
64 frames at 1280x720 and at 160x90.  Per shape: time per call (device events around `reps` calls on one stream; a call = one
memset + one kernel), the bytes a call must read (9 per pixel: two float planes and the ids) and the resulting GB/s, and whether
that working set fits the 256 MiB Infinity Cache (then repeated calls re-read it on-die and the figure is no HBM rate).  The
torch formulation — int64 Q32 depths, boolean planes, one masked sum per word — is compared for equality before anything is timed.
Usage: python tools/bench_verify.py [--reps 200] [--out profiles/verify_agreement.txt]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

INFINITY_CACHE = 256 * 2 ** 20


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


def torch_sums(R, ids, T, n_links, tol):
    """The 28 words per frame with torch operators: (N, 28) int64."""
    import torch
    q = lambda x: torch.floor(x.double() * 4294967296.0).long()   # noqa: E731
    valid = torch.isfinite(T) & (T > 0) & (T < 128)
    rendered = ids < n_links
    both = rendered & valid
    d = q(R) - q(torch.where(valid, T, torch.zeros_like(T)))
    a = d.abs()
    tq = int(np.floor(float(np.float32(tol)) * 4294967296.0))
    close, front = both & (a <= tq), both & (d > tq)
    cnt = lambda m: m.sum(dim=(1, 2))                             # noqa: E731
    words = [cnt(valid), cnt(rendered), torch.where(both, a, torch.zeros_like(a)).sum(dim=(1, 2)), cnt((ids >= n_links) & (ids < 255))]
    for l in range(n_links):
        m = ids == l
        words += [cnt(m), cnt(m & both), cnt(m & close), cnt(m & front)]
    words += [torch.zeros_like(words[0])] * (28 - len(words))
    return torch.stack(words, dim=1)


def main():
    import ctypes as C
    import torch
    from rope_s3d_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    lib = eng.load_library()
    n_links, tol, N = 6, 2.0 ** -5, 64
    lines = [f"rope_frame_agreement against torch, {torch.cuda.get_device_name(0)}, build {lib.rope_build_id().decode()}, "
             f"{args.reps} calls per figure (device events; a call = 1 memset + 1 kernel), {N} frames, {n_links} links, tol 2^-5 m",
             f"{'shape':<20}{'MB read':>9}{'fits L3':>9}{'kernel ms':>11}{'GB/s':>8}{'torch ms':>10}{'torch/kernel':>14}"]
    for (H, W) in ((720, 1280), (90, 160)):
        g = torch.Generator(device='cuda').manual_seed(H)
        R = torch.rand((N, H, W), device='cuda', generator=g) * 3 + 0.5
        T = R + (torch.randint(-2, 3, (N, H, W), device='cuda', generator=g).float() * tol)
        T[torch.rand((N, H, W), device='cuda', generator=g) < 0.1] = 0.0
        ids = torch.randint(0, 10, (N, H, W), device='cuda', generator=g, dtype=torch.uint8)
        ids[ids >= n_links] = 255                                 # 40 % background
        sums = torch.empty((N, 28), dtype=torch.int64, device='cuda')
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731

        def kernel():
            rc = lib.rope_frame_agreement(p(R), p(ids), p(T), N, H, W, n_links, tol, p(sums), stream)
            assert rc == 0, rc

        kernel()
        torch.cuda.synchronize()
        assert torch.equal(sums, torch_sums(R, ids, T, n_links, tol)), "the kernel's sums differ from the torch formulation"
        t_k = timed(kernel, args.reps)
        t_t = timed(lambda: torch_sums(R, ids, T, n_links, tol), max(10, args.reps // 10), warmup=2)
        nbytes = 9 * N * H * W
        lines.append(f"{f'{N} @ {W}x{H}':<20}{nbytes / 1e6:>9.2f}{'yes' if nbytes <= INFINITY_CACHE else 'no':>9}{t_k:>11.4f}"
                     f"{nbytes / t_k / 1e6:>8.0f}{t_t:>10.4f}{t_t / t_k:>14.1f}")
        del R, T, ids
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
