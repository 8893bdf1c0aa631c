"""CPU test of the audit itself (tests/trunk_audit.py): a plain fp32 evaluation of the runner's hops, stored at the offsets of evk_trunk_plan
with the engine's 16-bit roundings, must pass every derived bound in train and eval mode -- the reference alone satisfies them with no
element left out -- and defects of the size the audit exists for must be named at the quantity concerned."""
import pytest
import torch


@pytest.fixture(scope='module')
def case():
    from tests import trunk_audit as TA
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return TA.TrunkCase((2, 1, 1, 1), (16, 32, 64, 128), 3, 64, 96, seed=3, ill=True)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_fp32_evaluation_of_every_hop_is_inside_the_derived_bounds(case, training):
    from tests import trunk_audit as TA
    res = TA.emulate_engine(case, training)
    fails, lines, worst = TA.evaluate(case.audit(res, training))
    print('\n'.join(lines))
    assert not fails, '\n'.join(fails[:20])
    # the bounds are not slack by orders of magnitude: the 16-bit outputs come close to theirs somewhere
    assert max(v['y'][0] for v in worst.values()) > 0.3 and max(v['dy'][0] for v in worst.values()) > 0.2


@pytest.mark.parametrize('mutate,quantity', [('sum_gx', 'sum_gx'), ('bessel', 'running_var'), ('stats_row', 'sum'), ('gate', 'dy')])
def test_audit_names_the_defective_quantity(case, mutate, quantity):
    from tests import trunk_audit as TA
    res = TA.emulate_engine(case, True, mutate=mutate)
    fails, _, _ = TA.evaluate(case.audit(res, True))
    assert any(' %s:' % quantity in f for f in fails), fails[:10]
