"""GPU: the riders of Trainer.validate do not disturb each other.  Each rider's paragraph of validate's docstring
promises "behind every other key, and changing none"; here all of them run at once -- rigid refine, segment, object refine and
ICP started from the rigid fit -- against the runs that hold a part of them.  A key two runs share is the same float: ==, no
tolerance, since the shared keys come from the same launches on the same inputs."""
import pytest

pytestmark = pytest.mark.gpu

BASE = ['--evaluate', '--arch', 'HPLFlowNetShallow', '--pairs', '3', '--points', '256']
RIGID = ['--rigid-refine']
ICP = ['--baseline', 'icp', '--icp-init', 'rigid']
ALL = RIGID + ['--segment', '--object-refine'] + ICP
PARTS = {'rigid': RIGID, 'rigid+segment': RIGID + ['--segment'], 'rigid+icp': RIGID + ICP}


@pytest.mark.parametrize('batch', [[], ['--batch-size', '2'], ['--batch-size', '2', '--ragged']], ids=['one', 'equal', 'ragged'])
def test_all_riders_at_once_change_no_key_of_a_part(batch):
    from hplflownet_amd import engine
    whole = engine.main(BASE + batch + ALL)
    base = ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers']
    assert list(whole) == base + ['rigid_' + k for k in base] + list(engine.RIGID_STATS) + list(engine.SEGMENT_STATS) + \
        ['icp_' + k for k in base] + list(engine.ICP_STATS) + ['piecewise_' + k for k in base] + list(engine.OBJECT_STATS)
    for name, flags in PARTS.items():
        part = engine.main(BASE + batch + flags)
        assert set(part) < set(whole) and list(part) == [k for k in whole if k in part], name
        differ = {k: (part[k], whole[k]) for k in part if part[k] != whole[k]}
        print(name, 'keys', len(part), 'differ', differ)
        assert not differ, (name, differ)
