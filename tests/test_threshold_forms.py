"""Which kernel form the threshold stage sends a batch down (csrc/host_threshold.h: ThrPlan, launch_threshold) is what it was at the
commit tests/golden/fx_threshold_forms.json was recorded at.  Every form is exact, so parity with the oracle alone cannot see a batch
that silently takes another one; the tuple of nfc_stats that make_threshold_forms.py records per batch can."""
import pytest

from tests.golden import make_threshold_forms as forms
from tests.golden_util import load_json
from tests.test_gpu_parity import first_diff, oracle_run
from usrp_nfc_amd import api

pytestmark = pytest.mark.gpu

_ORACLE = {}   # (stream, av_window) -> (transitions, packets) of the C oracle


def _oracle(s):
    key = (s['stream'], s['params']['av_window'])
    if key not in _ORACLE:
        o = oracle_run(forms.stream(s['stream']), s['params'], api.NFC_IN_IQ_F32)
        _ORACLE[key] = (o.transitions(), o.packets())
    return _ORACLE[key]


@pytest.mark.parametrize('name', sorted(forms.SCENARIOS))
def test_threshold_form_is_the_recorded_one(monkeypatch, name):
    want = load_json('fx_threshold_forms.json')
    assert tuple(want['fields']) == forms.FIELDS
    tuples, tr, pk = forms.run(name, monkeypatch.setenv, monkeypatch.delenv)
    print('%s: %s' % (name, tuples))
    assert forms.SHOWS[name](want['scenarios'][name]), 'the record does not show the form this scenario is there for'
    assert tuples == want['scenarios'][name]
    want_tr, want_pk = _oracle(forms.SCENARIOS[name])
    d = first_diff(tr, want_tr)
    assert d is None, 'transition %s' % (d,)
    assert pk == want_pk and len(want_tr) > 100
