"""Time the native Inception-v3 forward against the stock-torch fp32 restatement (ATen / MIOpen) on the same GPU.

    python tools/bench_inception.py [--batches 8 64] [--iters 20] [--warmup 5] [--out profiles/inception_forward]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_inception.py --trace-only --batches 64
    python tools/bench_inception.py --families DIR/**/*kernel_trace.csv      (per-layer-family table from that trace)

Procedural weights (tests/inception_cases.py), 299 x 299.  Per batch size: HIP-event time of every forward (warm-up first,
native and ATen alternating), median / min / max, images per second and the whole-forward share of the fp32-MFMA floor
2 x 5.71 GFLOP x B / 157.3 TFLOP/s (an end-to-end figure, not a kernel's share of peak).  Writes <out>.json and <out>.txt.
--trace-only runs the native forward a few times with nothing else, for a profiler run of its own; the native launches of
one forward are then matched, in order, to the plan's layers to give the time per layer family."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
PEAK_FP32_MFMA = 157.3e12
MACS = 5.71e9


def family(op):
    if op[0] != 'conv':
        return 'pools'
    kh, kw, stride = op[8], op[9], op[10]
    if (kh, kw) == (3, 3):
        return '3x3 s%d' % stride
    return {(1, 1): '1x1', (5, 5): '5x5', (1, 7): '1x7/7x1', (7, 1): '1x7/7x1', (1, 3): '1x3/3x1', (3, 1): '1x3/3x1'}[(kh, kw)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def family_table(paths, batch):
    """Kernel-trace CSV(s) of a --trace-only run -> {family: (ms per forward, MACs per image)}: the inc_* launches repeat
    with the plan's period, so launch i belongs to plan op i mod len(ops)."""
    from tartangan_amd.models.inception import Inception3
    plan = Inception3().plan(299, 299)
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                if 'inc_' in r['Kernel_Name']:
                    rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp'])))
    rows.sort()
    n = len(plan.ops)
    assert rows and len(rows) % n == 0, (len(rows), n)
    reps = len(rows) // n
    out = {}
    for i, (s, e) in enumerate(rows[(reps - 1) * n:]):              # the last forward: steady state
        op = plan.ops[i]
        fam = family(op)
        macs = 0
        if op[0] == 'conv':
            _, _, _, _, cin, cout, h, w, kh, kw, stride, ph, pw = op[:13]
            macs = cout * cin * kh * kw * ((h + 2 * ph - kh) // stride + 1) * ((w + 2 * pw - kw) // stride + 1)
        t, m = out.get(fam, (0.0, 0))
        out[fam] = (t + (e - s) * 1e-6, m + macs)
    lines = ['family          ms/forward   GMAC/img   TFLOP/s   of fp32-MFMA peak   (batch %d)' % batch]
    for fam, (ms, macs) in sorted(out.items()):
        tf = 2 * macs * batch / (ms * 1e-3) / 1e12 if macs else 0.0
        lines.append('%-14s %10.3f %10.3f %9.1f %10.2f' % (fam, ms, macs / 1e9, tf, tf * 1e12 / PEAK_FP32_MFMA))
    return {k: {'ms': v[0], 'macs_per_image': v[1]} for k, v in out.items()}, lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', type=int, nargs='+', default=[8, 64])
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--out', default=None)
    p.add_argument('--trace-only', action='store_true')
    p.add_argument('--families', nargs='+', default=None, help='kernel-trace CSV files (globs) of a --trace-only run')
    args = p.parse_args()
    if args.families:
        paths = [q for g in args.families for q in glob.glob(g, recursive=True)]
        table, lines = family_table(paths, args.batches[-1])
        print('\n'.join(lines))
        if args.out:
            with open(args.out + '_families.json', 'w') as f:
                json.dump({'batch': args.batches[-1], 'families': table}, f, indent=1)
            with open(args.out + '_families.txt', 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    assert torch.cuda.is_available(), 'bench_inception needs the GPU (no CPU timing)'
    import inception_cases as IC
    from tartangan_amd.models.inception import Inception3
    state = IC.procedural_state(0)
    net = Inception3()
    net.load_state_dict(state)
    net = net.to('cuda')
    results, lines = [], []
    with torch.no_grad():
        if args.trace_only:
            x = IC.procedural_input(args.batches[-1], 299).to('cuda')
            for _ in range(3):
                net(x)
            torch.cuda.synchronize()
            return
        ref = IC.reference(state, torch.float32).to('cuda')
        for B in args.batches:
            x = IC.procedural_input(B, 299).to('cuda')
            got, want = net(x), ref(x)
            diff = max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(got, want))
            for fn in (lambda: net(x), lambda: ref(x)):
                timed(fn, 1, args.warmup)
            native, aten = [], []
            for _ in range(args.iters):                               # alternate, so that both see the same machine
                native += timed(lambda: net(x), 1, 0)
                aten += timed(lambda: ref(x), 1, 0)
            floor_ms = 2 * MACS * B / PEAK_FP32_MFMA * 1e3
            row = {'batch': B, 'iters': args.iters, 'max_rel_diff_vs_aten': diff, 'fp32_mfma_floor_ms': floor_ms}
            for name, t in (('native', native), ('aten', aten)):
                med = statistics.median(t)
                row[name] = {'median_ms': med, 'min_ms': min(t), 'max_ms': max(t), 'img_per_s': B / med * 1e3,
                             'fraction_of_fp32_mfma_floor': floor_ms / med}
                lines.append('B %3d %-6s median %8.3f ms (min %8.3f max %8.3f)  %8.1f img/s  %.3f of the fp32-MFMA floor'
                             % (B, name, med, min(t), max(t), B / med * 1e3, floor_ms / med))
            lines.append('B %3d native / aten time %.3f   max rel diff of (pool, logits) %.2e' % (B, row['native']['median_ms'] / row['aten']['median_ms'], diff))
            results.append(row)
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'input': '299x299', 'results': results}, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
