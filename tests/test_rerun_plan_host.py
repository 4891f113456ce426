"""The rounds of re-runs of the threshold stage as a host-only plan (usrp_nfc_amd/csrc/rerun_plan.h), checked without a GPU:
tools/rerun_plan_check drives failing_of / plan_round / pending_after with a model of the device through every chunk count 1 .. 12 and
every policy, and checks the partition, that no chunk goes back to the workgroup kernel, when the in-place form is switched off, the
pending list, the convergence bound the host enforces, the hand-written cases and the exactness guard (its header lists them)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rerun_plan_holds_its_properties_on_the_cpu(tmp_path):
    exe = tmp_path / 'rerun_plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'rerun_plan_check', 'main.cpp'), '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert 'every property held' in run.stdout, run.stdout


def test_the_plan_header_is_host_only():
    # no HIP include, nothing of the context: plain g++ compiles it (above), and the round rules are stated in it alone
    src = open(os.path.join(ROOT, 'usrp_nfc_amd', 'csrc', 'rerun_plan.h')).read()
    assert 'hip/' not in src and 'nfc_ctx' not in src
    host = open(os.path.join(ROOT, 'usrp_nfc_amd', 'csrc', 'host_threshold.h')).read()
    for rule in ('tried_wg[', 'ever_rerun[', 'ex_off =', 'lone_div <=', 'gflags[k] & 4'):
        assert rule in src and rule not in host, rule
