"""The refusals of the driver's options (hplflownet_amd.engine) as one table, texts included.

ARGV: command lines parse_args refuses -- at least one row per error site, one for the switch and one for the range where a site
has both -- with the message argparse prints (SystemExit 2, 'error: <text>' at the end of stderr).  The token DIR stands for an
existing directory, NODIR for a missing one.

CALLS: the programmatic side -- Trainer.validate on a reader without samples (nothing is launched), segment_options,
object_options, selfsup_options -- with the HplError text, or None where the call is taken: the ranges validate(rigid=...) and
validate(icp=...) leave to the op wrappers are rows of that kind.

`python tests/engine_refusals.py [ENGINE.py]` prints one line per row (call | row | exception type | text) and then --help at
COLUMNS=100, of the package's engine or of the engine.py named: two trees' listings are compared with diff."""
import contextlib
import importlib.util
import io
import os
import sys

INF = float('inf')

_K = ['--evaluate', '--dataset', 'KITTI']
_W = _K + ['--kitti-calib', 'DIR', '--write-kitti', 'DIR']
_D = _K + ['--dense']
_R = ['--evaluate', '--rigid-refine']
_S = _R + ['--segment']
_O = _S + ['--object-refine']
_I = ['--evaluate', '--baseline', 'icp']
_P = _I + ['--icp-metric', 'plane']
_L = ['--loss', 'selfsup']
_G = ['--dataset', 'KITTI', '--ground', 'plane']
_OS = ['--dataset', 'KITTI', '--outlier', 'statistical']
_OR = ['--dataset', 'KITTI', '--outlier', 'radius']

ARGV = [
    (['--write-kitti', 'DIR'], '--write-kitti applies to --evaluate --dataset KITTI with --kitti-calib DIR'),
    (_K + ['--write-kitti', 'DIR'], '--write-kitti applies to --evaluate --dataset KITTI with --kitti-calib DIR'),
    (['--write-footprint', '1'], '--write-footprint takes 0 .. 4 and applies to --write-kitti'),
    (_W + ['--write-size', '4', '4', '--write-footprint', '5'], '--write-footprint takes 0 .. 4 and applies to --write-kitti'),
    (['--write-size', '4', '4'], '--write-size takes two sizes >= 1 and applies to --write-kitti without --raw-root'),
    (_W + ['--write-size', '0', '4'], '--write-size takes two sizes >= 1 and applies to --write-kitti without --raw-root'),
    (_W + ['--raw-root', 'DIR', '--write-size', '4', '4'],
     '--write-size takes two sizes >= 1 and applies to --write-kitti without --raw-root'),
    (_W, '--write-kitti without --raw-root needs --write-size H W'),
    (['--batch-size', '4'], '--batch-size takes 1 .. 64 and applies to --evaluate (training takes one pair per step)'),
    (['--evaluate', '--batch-size', '65'], '--batch-size takes 1 .. 64 and applies to --evaluate (training takes one pair per step)'),
    (['--evaluate', '--batch-size', '0'], '--batch-size takes 1 .. 64 and applies to --evaluate (training takes one pair per step)'),
    (['--evaluate', '--train-batch-size', '2'],
     '--train-batch-size takes 1 .. 64 and applies to training (--evaluate batches with --batch-size)'),
    (['--train-batch-size', '65'], '--train-batch-size takes 1 .. 64 and applies to training (--evaluate batches with --batch-size)'),
    (['--ragged'], '--ragged applies to --evaluate with --batch-size >= 2'),
    (['--evaluate', '--ragged'], '--ragged applies to --evaluate with --batch-size >= 2'),
    (['--kitti-calib', 'DIR'], '--kitti-calib takes an existing directory and applies to --dataset KITTI'),
    (['--dataset', 'KITTI', '--kitti-calib', 'NODIR'], '--kitti-calib takes an existing directory and applies to --dataset KITTI'),
    (['--raw-root', 'DIR'], '--raw-root takes an existing directory and applies to --dataset FlyingThings3DSubset|KITTI'),
    (['--dataset', 'KITTI', '--raw-root', 'NODIR'],
     '--raw-root takes an existing directory and applies to --dataset FlyingThings3DSubset|KITTI'),
    (['--dataset', 'KITTI', '--raw-root', 'DIR', '--data-root', 'DIR'], '--raw-root and --data-root exclude each other'),
    (['--dataset', 'KITTI', '--raw-root', 'DIR'], '--raw-root with --dataset KITTI needs --kitti-calib DIR (every frame\'s P_rect_02)'),
    (['--device-transforms'], '--device-transforms applies to --dataset FlyingThings3DSubset|KITTI (synthetic pairs have no transform)'),
    (['--dense'], '--dense applies to --evaluate with --dataset FlyingThings3DSubset|KITTI'),
    (['--evaluate', '--dense'], '--dense applies to --evaluate with --dataset FlyingThings3DSubset|KITTI'),
    (['--dataset', 'KITTI', '--dense'], '--dense applies to --evaluate with --dataset FlyingThings3DSubset|KITTI'),
    (_K + ['--dense-fill', 'knn'], '--dense-fill applies to --dense'),
    (_D + ['--dense-k', '3'], '--dense-k takes 1 .. 8 and applies to --dense-fill knn'),
    (_D + ['--dense-fill', 'knn', '--dense-k', '9'], '--dense-k takes 1 .. 8 and applies to --dense-fill knn'),
    (_D + ['--dense-fill', 'knn', '--dense-k', '0'], '--dense-k takes 1 .. 8 and applies to --dense-fill knn'),
    (['--rigid-refine'], '--rigid-refine applies to --evaluate'),
    (['--evaluate', '--rigid-iters', '3'], '--rigid-iters takes 0 .. 16 and applies to --rigid-refine'),
    (_R + ['--rigid-iters', '17'], '--rigid-iters takes 0 .. 16 and applies to --rigid-refine'),
    (_R + ['--rigid-iters', '-1'], '--rigid-iters takes 0 .. 16 and applies to --rigid-refine'),
    (['--evaluate', '--rigid-tau', '0.1'], '--rigid-tau takes a finite value > 0 and applies to --rigid-refine'),
    (_R + ['--rigid-tau', '0'], '--rigid-tau takes a finite value > 0 and applies to --rigid-refine'),
    (_R + ['--rigid-tau', 'inf'], '--rigid-tau takes a finite value > 0 and applies to --rigid-refine'),
    (_R + ['--rigid-tau', 'nan'], '--rigid-tau takes a finite value > 0 and applies to --rigid-refine'),
    (['--evaluate', '--segment'], '--segment applies to --evaluate --rigid-refine'),
    (_R + ['--segment-eps', '1'], '--segment-eps takes a finite value > 0 and applies to --segment'),
    (_S + ['--segment-eps', 'inf'], '--segment-eps takes a finite value > 0 and applies to --segment'),
    (_S + ['--segment-eps', '0'], '--segment-eps takes a finite value > 0 and applies to --segment'),
    (_R + ['--segment-dv', '1'], '--segment-dv takes a value > 0 and applies to --segment'),
    (_S + ['--segment-dv', '0'], '--segment-dv takes a value > 0 and applies to --segment'),
    (_S + ['--segment-dv', 'nan'], '--segment-dv takes a value > 0 and applies to --segment'),
    (_R + ['--segment-min-points', '5'], '--segment-min-points takes a value >= 1 and applies to --segment'),
    (_S + ['--segment-min-points', '0'], '--segment-min-points takes a value >= 1 and applies to --segment'),
    (_R + ['--object-refine'], '--object-refine applies to --evaluate --rigid-refine --segment'),
    (['--evaluate', '--object-refine'], '--object-refine applies to --evaluate --rigid-refine --segment'),
    (_S + ['--object-iters', '2'], '--object-iters takes 0 .. 16 and applies to --object-refine'),
    (_O + ['--object-iters', '17'], '--object-iters takes 0 .. 16 and applies to --object-refine'),
    (_S + ['--object-tau', '0.2'], '--object-tau takes a finite value > 0 and applies to --object-refine'),
    (_O + ['--object-tau', '0'], '--object-tau takes a finite value > 0 and applies to --object-refine'),
    (_O + ['--object-tau', 'inf'], '--object-tau takes a finite value > 0 and applies to --object-refine'),
    (['--baseline', 'icp'], '--baseline applies to --evaluate'),
    (['--evaluate', '--icp-iters', '3'], '--icp-iters takes 0 .. 64 and applies to --baseline icp'),
    (_I + ['--icp-iters', '65'], '--icp-iters takes 0 .. 64 and applies to --baseline icp'),
    (['--evaluate', '--icp-max-dist', '1'], '--icp-max-dist takes a finite value > 0 and applies to --baseline icp'),
    (_I + ['--icp-max-dist', '0'], '--icp-max-dist takes a finite value > 0 and applies to --baseline icp'),
    (_I + ['--icp-max-dist', 'inf'], '--icp-max-dist takes a finite value > 0 and applies to --baseline icp'),
    (['--evaluate', '--icp-tau', '1'], '--icp-tau takes a finite value > 0 and applies to --baseline icp'),
    (_I + ['--icp-tau', 'nan'], '--icp-tau takes a finite value > 0 and applies to --baseline icp'),
    (['--evaluate', '--icp-init', 'identity'], '--icp-init applies to --baseline icp'),
    (_I + ['--icp-init', 'rigid'], '--icp-init rigid starts from the fit of --rigid-refine'),
    (['--evaluate', '--icp-metric', 'plane'], '--icp-metric applies to --baseline icp'),
    (_I + ['--icp-normals-k', '8'], '--icp-normals-k takes 3 .. 32 and applies to --icp-metric plane'),
    (_I + ['--icp-metric', 'point', '--icp-normals-k', '8'], '--icp-normals-k takes 3 .. 32 and applies to --icp-metric plane'),
    (_P + ['--icp-normals-k', '2'], '--icp-normals-k takes 3 .. 32 and applies to --icp-metric plane'),
    (_P + ['--icp-normals-k', '33'], '--icp-normals-k takes 3 .. 32 and applies to --icp-metric plane'),
    (_I + ['--icp-normals-radius', '1'], '--icp-normals-radius takes a finite value > 0 and applies to --icp-metric plane'),
    (_P + ['--icp-normals-radius', '0'], '--icp-normals-radius takes a finite value > 0 and applies to --icp-metric plane'),
    (_P + ['--icp-normals-radius', 'inf'], '--icp-normals-radius takes a finite value > 0 and applies to --icp-metric plane'),
    (['--evaluate'] + _L, '--loss applies to training (--evaluate reports the supervised metrics)'),
    (['--selfsup-k', '3'], '--selfsup-k takes 1 .. 8 and applies to --loss selfsup'),
    (_L + ['--selfsup-k', '0'], '--selfsup-k takes 1 .. 8 and applies to --loss selfsup'),
    (_L + ['--selfsup-k', '9'], '--selfsup-k takes 1 .. 8 and applies to --loss selfsup'),
    (['--selfsup-chamfer-weight', '1'], '--selfsup-chamfer-weight takes a finite value >= 0 and applies to --loss selfsup'),
    (_L + ['--selfsup-chamfer-weight', '-1'], '--selfsup-chamfer-weight takes a finite value >= 0 and applies to --loss selfsup'),
    (['--selfsup-smooth-weight', '1'], '--selfsup-smooth-weight takes a finite value >= 0 and applies to --loss selfsup'),
    (_L + ['--selfsup-smooth-weight', 'inf'], '--selfsup-smooth-weight takes a finite value >= 0 and applies to --loss selfsup'),
    (['--selfsup-native'], '--selfsup-native applies to --loss selfsup'),
    (['--ground', 'plane'], '--ground applies to --dataset KITTI'),
    (['--dataset', 'KITTI', '--ground-tau', '0.1'], '--ground-tau takes a finite value > 0 and applies to --ground plane'),
    (_G + ['--ground-tau', '0'], '--ground-tau takes a finite value > 0 and applies to --ground plane'),
    (['--dataset', 'KITTI', '--ground-cut', '0.1'], '--ground-cut takes a finite value >= 0 and applies to --ground plane'),
    (_G + ['--ground-cut', '-1'], '--ground-cut takes a finite value >= 0 and applies to --ground plane'),
    (_G + ['--ground-cut', 'inf'], '--ground-cut takes a finite value >= 0 and applies to --ground plane'),
    (['--dataset', 'KITTI', '--ground-hyps', '8'], '--ground-hyps takes 1 .. 1024 and applies to --ground plane'),
    (_G + ['--ground-hyps', '1025'], '--ground-hyps takes 1 .. 1024 and applies to --ground plane'),
    (['--dataset', 'KITTI', '--ground-tilt', '8'], '--ground-tilt takes 0 <= DEG < 90 and applies to --ground plane'),
    (_G + ['--ground-tilt', '90'], '--ground-tilt takes 0 <= DEG < 90 and applies to --ground plane'),
    (_G + ['--ground-tilt', 'nan'], '--ground-tilt takes 0 <= DEG < 90 and applies to --ground plane'),
    (['--dataset', 'KITTI', '--ground-up', '0', '1', '0'],
     '--ground-up takes three finite numbers, not all zero, and applies to --ground plane'),
    (_G + ['--ground-up', '0', '0', '0'], '--ground-up takes three finite numbers, not all zero, and applies to --ground plane'),
    (_G + ['--ground-up', '0', 'inf', '0'], '--ground-up takes three finite numbers, not all zero, and applies to --ground plane'),
    (_G + ['--ground-up', '0', 'nan', '0'], '--ground-up takes three finite numbers, not all zero, and applies to --ground plane'),
    (['--voxel', '0.2'], '--voxel applies to --dataset KITTI'),
    (['--dataset', 'KITTI', '--voxel', '0'], '--voxel takes a finite value > 0'),
    (['--dataset', 'KITTI', '--voxel', 'inf'], '--voxel takes a finite value > 0'),
    (['--dataset', 'KITTI', '--voxel-mode', 'nearest'], '--voxel-mode applies to --voxel'),
    (['--outlier', 'radius'], '--outlier applies to --dataset KITTI'),
    (_OR + ['--outlier-k', '8'], '--outlier-k takes 1 .. 32 and applies to --outlier statistical'),
    (_OS + ['--outlier-k', '33'], '--outlier-k takes 1 .. 32 and applies to --outlier statistical'),
    (['--dataset', 'KITTI', '--outlier-radius', '1'], '--outlier-radius takes a finite value > 0 and applies to --outlier'),
    (_OR + ['--outlier-radius', '0'], '--outlier-radius takes a finite value > 0 and applies to --outlier'),
    (_OR + ['--outlier-std-ratio', '1'], '--outlier-std-ratio takes a finite value >= 0 and applies to --outlier statistical'),
    (_OS + ['--outlier-std-ratio', '-1'], '--outlier-std-ratio takes a finite value >= 0 and applies to --outlier statistical'),
    (_OS + ['--outlier-min-neighbors', '2'], '--outlier-min-neighbors takes an int >= 1 and applies to --outlier radius'),
    (_OR + ['--outlier-min-neighbors', '0'], '--outlier-min-neighbors takes an int >= 1 and applies to --outlier radius'),
    (_OR + ['--outlier-min-neighbors', str(2 ** 31)], '--outlier-min-neighbors takes an int >= 1 and applies to --outlier radius'),
    (['--fps', '8'], '--fps applies to --dataset KITTI'),
    (['--dataset', 'KITTI', '--fps', '0'], '--fps takes an int >= 1'),
    # two faults on one line: the one that is heard first
    (['--rigid-refine', '--rigid-iters', '17'], '--rigid-refine applies to --evaluate'),
    (['--evaluate', '--segment', '--segment-eps', '0'], '--segment applies to --evaluate --rigid-refine'),
    (_I + ['--icp-init', 'rigid', '--icp-normals-k', '8'], '--icp-init rigid starts from the fit of --rigid-refine'),
    (['--write-footprint', '9', '--batch-size', '0'], '--write-footprint takes 0 .. 4 and applies to --write-kitti'),
    (['--fps', '0', '--voxel', '0'], '--voxel applies to --dataset KITTI'),
]

_RIGID = {'iters': 2, 'tau': 0.1}
_ICP_TAKES = ('validate: icp takes {\'iters\': T, \'max_dist\': d, \'tau\': tau, \'init\': \'identity\' | \'rigid\', \'metric\': '
              '\'point\' | \'plane\'[, \'normals_k\': K, \'normals_radius\': R with \'plane\']}, got ')
_SEG_TAKES = 'validate: segment takes {\'eps\': e, \'dv\': v, \'min_points\': m}, got '
_SEG_NEEDS = 'validate: segment needs eps finite and > 0, dv > 0 and min_points >= 1, got '
_OBJ_TAKES = 'validate: objects takes {\'iters\': T, \'tau\': tau}, got '
_OBJ_NEEDS = 'validate: objects needs iters in 0 .. 16 and tau finite and > 0, got '
_SS_TAKES = 'Trainer: selfsup takes {\'k\': k, \'w_chamfer\': w, \'w_smooth\': w}, got '
_SS_NEEDS = 'Trainer: selfsup needs k in 1 .. 8 (0 with w_smooth = 0) and finite weights >= 0, got '

# (call, positional arguments, keyword arguments, the HplError's text or None: taken)
CALLS = [
    ('validate', (), {'dense_fill': 'knn'}, 'validate: dense_fill applies to dense=True'),
    ('validate', (), {'rigid': {'iterations': 2}}, 'validate: rigid takes {\'iters\': T, \'tau\': tau}, got {\'iterations\': 2}'),
    ('validate', (), {'rigid': 3}, 'validate: rigid takes {\'iters\': T, \'tau\': tau}, got 3'),
    ('validate', (), {'rigid': {'iters': 99, 'tau': -1.0}}, None),           # (ops.rigid_fit's to refuse)
    ('validate', (), {'segment': {}}, 'validate: segment applies to rigid'),
    ('validate', (), {'rigid': _RIGID, 'segment': {'eps': 0}}, _SEG_NEEDS + '{\'eps\': 0}'),
    ('validate', (), {'rigid': _RIGID, 'segment': {'iters': 2}}, _SEG_TAKES + '{\'iters\': 2}'),
    ('validate', (), {'objects': {}}, 'validate: objects applies to rigid with segment'),
    ('validate', (), {'rigid': _RIGID, 'objects': {}}, 'validate: objects applies to rigid with segment'),
    ('validate', (), {'rigid': _RIGID, 'segment': {}, 'objects': {'iters': 17}}, _OBJ_NEEDS + '{\'iters\': 17}'),
    ('validate', (), {'rigid': _RIGID, 'segment': {}, 'objects': {}, 'icp': {'init': 'rigid'}}, None),
    ('validate', (), {'icp': 3}, _ICP_TAKES + '3'),
    ('validate', (), {'icp': {'rounds': 2}}, _ICP_TAKES + '{\'rounds\': 2}'),
    ('validate', (), {'icp': {'init': 'flow'}}, _ICP_TAKES + '{\'init\': \'flow\'}'),
    ('validate', (), {'icp': {'metric': 'line'}}, _ICP_TAKES + '{\'metric\': \'line\'}'),
    ('validate', (), {'icp': {'normals_k': 8}}, _ICP_TAKES + '{\'normals_k\': 8}'),
    ('validate', (), {'icp': {'metric': 'point', 'normals_radius': 1.0}}, _ICP_TAKES + '{\'metric\': \'point\', \'normals_radius\': 1.0}'),
    ('validate', (), {'icp': {'init': 'rigid'}}, 'validate: icp init \'rigid\' starts from the rigid fit: it takes rigid'),
    ('validate', (), {'icp': {'iters': 999, 'max_dist': -1.0, 'metric': 'plane', 'normals_k': 99}}, None),   # (ops.icp's to refuse)
    ('segment_options', (3,), {}, _SEG_TAKES + '3'),
    ('segment_options', ({'eps': 1.0, 'iters': 2},), {}, _SEG_TAKES + '{\'eps\': 1.0, \'iters\': 2}'),
    ('segment_options', ({'eps': 0},), {}, _SEG_NEEDS + '{\'eps\': 0}'),
    ('segment_options', ({'eps': INF},), {}, _SEG_NEEDS + '{\'eps\': inf}'),
    ('segment_options', ({'dv': 0},), {}, _SEG_NEEDS + '{\'dv\': 0}'),
    ('segment_options', ({'dv': float('nan')},), {}, _SEG_NEEDS + '{\'dv\': nan}'),
    ('segment_options', ({'min_points': 0},), {}, _SEG_NEEDS + '{\'min_points\': 0}'),
    ('segment_options', ({},), {}, None),
    ('object_options', (3, _RIGID), {}, _OBJ_TAKES + '3'),
    ('object_options', ({'eps': 1},  _RIGID), {}, _OBJ_TAKES + '{\'eps\': 1}'),
    ('object_options', ({'iters': 17}, _RIGID), {}, _OBJ_NEEDS + '{\'iters\': 17}'),
    ('object_options', ({'iters': -1}, _RIGID), {}, _OBJ_NEEDS + '{\'iters\': -1}'),
    ('object_options', ({'tau': 0}, _RIGID), {}, _OBJ_NEEDS + '{\'tau\': 0}'),
    ('object_options', ({'tau': INF}, _RIGID), {}, _OBJ_NEEDS + '{\'tau\': inf}'),
    ('object_options', ({}, {'iters': 99, 'tau': 0.1}), {}, _OBJ_NEEDS + '{}'),       # (the default is the rigid fit's value)
    ('selfsup_options', ('nope', None), {}, 'Trainer: loss is \'epe3d\' or \'selfsup\', got \'nope\''),
    ('selfsup_options', ('epe3d', {}), {}, 'Trainer: selfsup options apply to loss=\'selfsup\''),
    ('selfsup_options', ('selfsup', 3), {}, _SS_TAKES + '3'),
    ('selfsup_options', ('selfsup', {'weight': 1}), {}, _SS_TAKES + '{\'weight\': 1}'),
    ('selfsup_options', ('selfsup', {'k': 9}), {}, _SS_NEEDS + '{\'k\': 9}'),
    ('selfsup_options', ('selfsup', {'k': True}), {}, _SS_NEEDS + '{\'k\': True}'),
    ('selfsup_options', ('selfsup', {'k': 2.0}), {}, _SS_NEEDS + '{\'k\': 2.0}'),
    ('selfsup_options', ('selfsup', {'k': 0}), {}, _SS_NEEDS + '{\'k\': 0}'),
    ('selfsup_options', ('selfsup', {'w_chamfer': -1}), {}, _SS_NEEDS + '{\'w_chamfer\': -1}'),
    ('selfsup_options', ('selfsup', {'w_smooth': INF}), {}, _SS_NEEDS + '{\'w_smooth\': inf}'),
    ('selfsup_options', ('selfsup', {'k': 0, 'w_smooth': 0}), {}, None),
]


class _NoSamples(object):
    has_cameras = True

    def __len__(self):
        return 0


def argv_verdict(engine, argv, directory):
    """(exception type's name, text) of parse_args(argv): ('SystemExit', argparse's message) for a refusal."""
    missing = os.path.join(directory, 'missing')
    argv = [{'DIR': directory, 'NODIR': missing}.get(x, x) for x in argv]
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            engine.parse_args(argv)
    except SystemExit as e:
        text = err.getvalue()
        return 'SystemExit %s' % (e.code,), text[text.index(': error: ') + 9:].rstrip('\n').replace(missing, 'NODIR').replace(directory, 'DIR')
    return 'taken', ''


def call_verdict(engine, name, args, kw):
    """(exception type's name, text) of one programmatic call; ('taken', '') where nothing is raised."""
    import torch
    if name == 'validate':
        tr = engine.Trainer.__new__(engine.Trainer)
        tr.model, tr.device = torch.nn.Identity(), torch.device('cpu')
        fn, args = tr.validate, (_NoSamples(),)
    else:
        fn = getattr(engine, name)
    try:
        fn(*args, **kw)
    except Exception as e:      # noqa: BLE001  (the listing shows whatever comes out)
        return type(e).__name__, str(e)
    return 'taken', ''


def help_text(engine, columns=100):
    old = os.environ.get('COLUMNS')
    os.environ['COLUMNS'] = str(columns)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out), contextlib.suppress(SystemExit):
            engine.parse_args(['--help'])
    finally:
        os.environ.pop('COLUMNS') if old is None else os.environ.__setitem__('COLUMNS', old)
    return out.getvalue()


def _main(argv):
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if argv:
        spec = importlib.util.spec_from_file_location('hplflownet_amd._engine_listed', argv[0])
        engine = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(engine)
    else:
        from hplflownet_amd import engine
    with tempfile.TemporaryDirectory() as d:
        for row, _ in ARGV:
            print('parse_args | %s | %s | %s' % ((' '.join(row),) + argv_verdict(engine, row, d)))
    for name, args, kw, _ in CALLS:
        print('%s | %s | %s | %s' % ((name, ', '.join([repr(x) for x in args] + ['%s=%r' % i for i in kw.items()])) + call_verdict(engine, name, args, kw)))
    print('==== --help, COLUMNS=100')
    sys.argv[0] = 'engine.py'
    print(help_text(engine))


if __name__ == '__main__':
    _main(sys.argv[1:])
