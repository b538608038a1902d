#!/usr/bin/env python
"""GPU: the per-object rigid fits of a segmented flow, read-back form against device form (hpl_object_fit) --
the table of profiles/object_fit_bench.txt.

Forms: flownet.segment_motion(object_fits=True) -- one read-back of obj_info, an argsort per pair and ops.rigid_fit over 64
objects a call --, flownet.segment_motion(object_fits='device') -- one ops.object_fit call, no read-back --, and
object_fits=False (what both share: the ego fit and ops.motion_segment).  Shapes: tests/segment_oracle.py's scene at 8 192
points (6 objects); a dense frame of 450 000 points with 209 boxes; a batch of 16 sampled pairs; and the worst case of the
design, 450 000 points in ONE object, where ops.object_fit is timed against ops.rigid_fit on the same points, with the sizes
between for the member count at which the two cross.

Every form ends in a synchronisation (the read-back form has one inside), so the clock is the host's around --calls calls.  The
forms are interleaved, twice, in one process; the table gives the median, the fastest and the slowest of all repeats per
call, and the kernels a call launches as the profiler counts them.  --out FILE also writes the table there."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def interleaved(forms, calls, repeats, warmup):
    """{name: (median, fastest, slowest) us per call}: the forms in turn, the whole round twice."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in forms}
    for _ in range(2):
        for k, fn in forms.items():
            out[k].extend(timed(fn, calls) for _ in range(repeats))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in out.items()}


def kernels_of(fn):
    """The kernels one call launches, as the profiler counts them (None where it cannot)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and
                'memset' not in e.name.lower())
        return n or None
    except Exception:                            # noqa: BLE001 (a profiler that is not there: the table says so)
        return None


def dense_frame(n, seed):
    """A static background under the tests' ego-motion and 11 x 19 boxes of 1 m with 480 points and a flow of their own each."""
    import segment_oracle
    r = np.random.RandomState(seed)
    centres = [(x, 0.0, z) for x in np.arange(-14.0, 14.1, 2.8) for z in np.arange(3.0, 34.0, 1.7)]
    per = 480
    nb = n - per * len(centres)
    p = [np.stack([r.uniform(-15, 15, nb), r.uniform(-2, 2, nb), r.uniform(2, 35, nb)])]
    for c in centres:
        p.append(np.asarray(c)[:, None] + r.uniform(-0.5, 0.5, (3, per)))
    p = np.concatenate(p, 1)
    f = segment_oracle.TRUE_R @ p + segment_oracle.TRUE_T[:, None] - p + 0.01 * r.normal(size=p.shape)
    for k in range(len(centres)):
        f[:, nb + k * per:nb + (k + 1) * per] += np.array([[1.0 + 0.01 * k], [0.0], [0.5]])
    order = r.permutation(n)
    return p[:, order].astype(np.float32), f[:, order].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import segment_oracle
    import hplflownet_amd as H
    from hplflownet_amd import ops
    dev = torch.device('cuda:0')
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per call, host clock around %d calls ending in a synchronisation: median (fastest .. slowest) of 2 x %d repeats, the '
             'forms interleaved, %d warm-up calls; kernels: what one call launches' % (a.calls, a.repeats, a.warmup), '']

    def say(row):
        lines.append(row)
        print(row, flush=True)

    def to(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    kw = dict(segment_oracle.SCENE_KW)
    shapes = []
    p, f = segment_oracle.scene(8192)[:2]
    shapes.append(('scene, N = 8192', to(p), to(f).t().contiguous().t(), None, kw))
    p, f = dense_frame(450000, 7)
    shapes.append(('dense frame, N = 450000', to(p), to(f).t().contiguous().t(), None, dict(kw, eps=0.5)))
    parts = [segment_oracle.scene(8192, 1 + b)[:2] for b in range(16)]
    shapes.append(('16 pairs of N = 8192', to(np.concatenate([x[0] for x in parts], 1)),
                   to(np.concatenate([x[1] for x in parts], 1)).t().contiguous().t(), [8192] * 16, kw))
    say('flownet.segment_motion(pc, flow, object_fits=...), 4 reweighted solves')
    for name, pc, flow, counts, skw in shapes:
        forms = {'False': lambda: H.segment_motion(pc, flow, counts, **skw),
                 'True': lambda: H.segment_motion(pc, flow, counts, object_fits=True, **skw),
                 "'device'": lambda: H.segment_motion(pc, flow, counts, object_fits='device', **skw)}
        t = interleaved(forms, a.calls, a.repeats, a.warmup)
        found = H.segment_motion(pc, flow, counts, **skw)[3].cpu().numpy()
        say('%s: %d objects, %d points in objects' % (name, int(found[:, 1].sum()), int(found[:, 2].sum())))
        for k in forms:
            say('    object_fits=%-9s %10.1f (%.1f .. %.1f)   kernels %s' % ((k,) + t[k] + (kernels_of(forms[k]),)))
        say('    the object fits alone: read-back form %.1f, device form %.1f (x %.2f)' % (
            t['True'][0] - t['False'][0], t["'device'"][0] - t['False'][0],
            (t['True'][0] - t['False'][0]) / max(t["'device'"][0] - t['False'][0], 1e-9)))
    say('')
    say('ONE object of n members: ops.object_fit (one workgroup walks n / 1024 spans a round) against ops.rigid_fit on the same points')
    p, f = dense_frame(450000, 8)
    for n in (1024, 4096, 16384, 65536, 131072, 262144, 450000):
        pc, flow = to(p[:, :n]), to(f[:, :n]).t().contiguous().t()
        labels = torch.zeros(n, dtype=torch.int32, device=dev)
        forms = {'rigid_fit': lambda: ops.rigid_fit(pc, flow, iters=4, tau=0.1),
                 'object_fit': lambda: ops.object_fit(pc, flow, labels, max_objects=1, iters=4, tau=0.1)}
        t = interleaved(forms, a.calls, a.repeats, a.warmup)
        say('    n = %6d: ops.rigid_fit %9.1f (%.1f .. %.1f) kernels %s   ops.object_fit %9.1f (%.1f .. %.1f) kernels %s   x %.2f' % (
            (n,) + t['rigid_fit'] + (kernels_of(forms['rigid_fit']),) + t['object_fit'] + (kernels_of(forms['object_fit']),) +
            (t['object_fit'][0] / t['rigid_fit'][0],)))
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
