"""Print the launch plans of a tree, one line per recorded op: the proof that a restructuring of the plan recorders changed no launch.

    python tools/plan_dump.py [--tree DIR] > dump.txt        (on the GPU; run it on both trees and diff the outputs)

Plans: all four models; 'f16x2', 'bf16x3', 'fp32' (and 'fp8' for qarv_base); the pipeline groups of B = 1 and B = 5 at 64x128 and of
B = 8 at 512x768; the coding kinds and the eval kinds on the whole batch; for qarv_base also the per-image-lambda ('vec') plans and
side_streams on / off.  A line holds the op's label, its entry point, the side-stream flag and every argument: integers and floats as
they are, a descriptor as its fields, and every address as the index of its first appearance in that plan (so the dump does not
depend on where the allocator put a buffer, only on which launches share one).  --tree: the tree whose package is imported
(default: the one this file is in)."""
import argparse
import ctypes
import os
import sys


def dump_plan(pl, out):
    seen = {}

    def addr(a):
        if not a:
            return '-'
        return f'@{seen.setdefault(int(a), len(seen))}'

    def fields(d):
        vals = []
        for name, t in d._fields_:
            v = getattr(d, name)
            vals.append(f'{name}={addr(v) if t is ctypes.c_void_p else v!r}')
        return '{' + ' '.join(vals) + '}'

    for fn, args, label, side in pl.ops:
        if not callable(fn):                                # a stream-ordering entry: (side waits for main, event)
            out.append(f'{label} ORDER {int(side)} {int(args[0])} {addr(args[1])}')
            continue
        vals = []
        for a, t in zip(args, fn.argtypes[:-1]):
            if t in (ctypes.c_float, ctypes.c_double):
                vals.append(repr(float(a)))
            elif t in (ctypes.c_int, ctypes.c_long):
                vals.append(str(int(a)))
            elif a is None or isinstance(a, int):
                vals.append(addr(a))
            else:                                           # byref() of a descriptor the plan keeps
                vals.append(fields(a._obj))
        out.append(f'{label} {fn.lvae_name} {int(side)} ' + ' '.join(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tree = os.path.abspath(ap.parse_args().tree)
    sys.path.insert(0, os.path.join(tree, 'lossy-vae_amd'))
    import torch
    import lvae
    out = []
    for name in ('qarv_base', 'qres34m', 'qres34m_lossless', 'qres17m'):
        qarv = name == 'qarv_base'
        torch.manual_seed(0)
        m = lvae.get_model(name).to('cuda:0').eval()
        m.compress_mode()
        for prec in ('f16x2', 'bf16x3', 'fp32') + (('fp8',) if qarv else ()):
            m.set_gemm_precision(prec)
            for B, H, W in ((1, 64, 128), (5, 64, 128), (8, 512, 768)):
                dec_size = (H // 64, W // 64) if qarv else (H, W)
                jobs = [(k, n, (H, W) if k == 'enc' else dec_size) for k in ('enc', 'dec') for n in sorted({n for _, n in m._groups(B, k)})]
                jobs += [('ence', B, (H, W)), ('encb', B, (H, W)), ('evald', B, dec_size)] if qarv else [('eval', B, (H, W))]
                for side in ((True, False) if qarv else (None,)):
                    for vec in ((False, True) if qarv else (None,)):
                        for kind, n, (a, b) in jobs:
                            if qarv:
                                if kind in ('dec', 'evald') and not side:
                                    continue                # decode plans record nothing on a side stream
                                m.side_streams = side
                            pl = m._plan(kind, n, a, b, vec=vec) if qarv else m._plan(kind, n, a, b)
                            out.append(f'# {name} {prec} {kind} n={n} {a}x{b}' + (f' side_streams={int(side)} vec={int(vec)}' if qarv else ''))
                            dump_plan(pl, out)
                            m._plans.clear()
    print('\n'.join(out))


if __name__ == '__main__':
    main()
