"""CPU: the connection table's directed cases (tests/conntrack_cases.py) reach what they are named
for, on the model and on the host form; the toy firewall drives the model packet by packet and
batch-wise to the same verdicts and the same map; and the model and the host form replay the
reference's reload and ICMP tests (tests/golden/conntrack_reload.json)."""
import json
import os

import numpy as np
import pytest

from nebula_amd import _lib as L
from nebula_amd import firewall as F

import conntrack_cases as K
import conntrack_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.all_cases()


def test_the_list_covers_every_directed_condition():
    names = " | ".join(c.name for c in CASES)
    for word in ("one home slot", "wraps", "behind a tombstone", "one field", "garbage", "4-in-6", "ICMP", "three timeouts",
                 "larger Expires", "STALE", "64 copies", "FULL by capacity", "FULL by tombstones", "evict", "compaction",
                 "status != OK", "work_cap"):
        assert word in names, word


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_reaches_its_condition_on_the_host_form(case):
    moved = []
    with F.Conntrack(None, case.capacity, seed=K.SEED, max_batch=case.max_batch) as ct:
        R.play(case.steps, R.Model(case.capacity), R.HostRunner(ct),
               after_step=lambda step, before: moved.append(before.tobytes() != ct.dump().tobytes()))
        case.reached(ct)
    if any(s[0] == "compact" for s in case.steps) and case.capacity > 1:
        assert any(moved)  # slot contents change


def test_one_field_variants_are_all_there():
    b4, b6, var = K.one_field_variants()
    w = F.key_words(np.concatenate([b4, b6, var]))
    assert len(w) == 23
    for base, rows in ((w[0], w[2:10]), (w[1], w[10:22])):
        for r in rows:  # one key word differs, in the bits of one field
            d = [int(a) ^ int(b) for a, b in zip(base, r)]
            assert sum(x != 0 for x in d) == 1
            x = [v for v in d if v][0]
            assert bin(x).count("1") <= 4
    assert int(w[22][4]) ^ int(w[0][4]) == (4 ^ 6) << 40 and list(w[22][:4]) == list(w[0][:4])  # family alone


def drive(fwall, batches, by_packet):
    out = []
    for fw, incoming, now, rules in batches:
        if rules is not None:
            fwall.reload(rules)
        if by_packet:
            out.append([fwall.drop_packet(fw[i], incoming, now) for i in range(len(fw))])
        else:
            out.append(fwall.drop_batch(fw, incoming, now))
    return out


def traffic(rng, nbatches):
    keys = K.universe(24)
    keys["local_port"] = 100 + np.arange(24) % 5
    keys["remote_port"] = 200 + np.arange(24) % 3
    rule_sets = [{(True, 0, 100), (False, 17, 0)}, {(True, 6, 0), (False, 0, 201)}, {(True, 0, 0)}, set()]
    out, now = [], K.T0
    for b in range(nbatches):
        now += int(rng.integers(1, R.UDP_NS))
        fw = keys[rng.integers(0, 24, int(rng.integers(1, 40)))]
        out.append((fw, bool(rng.integers(0, 2)), now, rule_sets[int(rng.integers(0, 4))] if b % 7 == 6 else None))
    return rule_sets[0], out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_packet_by_packet_and_batch_wise_agree(seed):
    rules, batches = traffic(np.random.default_rng(seed), 60)
    a, b = R.ToyFirewall(R.Model(64), rules), R.ToyFirewall(R.Model(64), rules)
    pa, pb = drive(a, batches, True), drive(b, batches, False)
    assert pa == pb
    assert a.ct.snapshot() == b.ct.snapshot() and a.wheel == b.wheel
    assert any(not all(p) for p in pa) and any(all(p) for p in pa) and len(a.wheel) > 4


def test_batch_wise_on_the_host_form_agrees_with_the_model():
    rules, batches = traffic(np.random.default_rng(9), 60)
    with F.Conntrack(None, 64, seed=K.SEED, max_batch=64) as ct:
        a, b = R.ToyFirewall(R.Model(64), rules), R.ToyFirewall(R.HostTableAsModel(ct), rules)
        assert drive(a, batches, True) == drive(b, batches, False)
        assert a.ct.snapshot() == b.ct.snapshot() and a.wheel == b.wheel


class GoldenFirewall(R.ToyFirewall):
    """The rule tables' answers come from the recorded step."""
    answers = {"in": False, "out": False}

    def match(self, rec, incoming):
        return self.answers["in" if incoming else "out"]


def replay_golden(make):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "conntrack_reload.json")))
    t = g["timeouts_ns"]
    for script in g["scripts"]:
        p = script["packet"]
        fw = F.fw_packets([(p["local"], p["remote"], p["local_port"], p["remote_port"], p["protocol"])], p["fragment"])
        for by_packet in (True, False):
            with make(t["tcp"], t["udp"], t["default"]) as (ct, _):
                fwall = GoldenFirewall(ct, ())
                for k, step in enumerate(script["steps"]):
                    if step["reset"]:  # resetConntrack
                        ct.evict(fw, 0, force=True)
                    ct.set_rules_version(step["version"])
                    fwall.answers = step["rules"]
                    passes = fwall.drop_packet(fw[0], step["incoming"], K.T0 + k) if by_packet else \
                        fwall.drop_batch(fw, step["incoming"], K.T0 + k)[0]
                    assert passes == (step["error"] is None), (script["name"], step["note"])


class _Ctx:
    def __init__(self, obj, close):
        self.obj, self.close = obj, close

    def __enter__(self):
        return self.obj, self.close

    def __exit__(self, *exc):
        self.close()


def test_model_replays_the_reference_reload_and_icmp_tests():
    replay_golden(lambda tcp, udp, dflt: _Ctx(R.Model(4, tcp, udp, dflt), lambda: None))


def test_host_form_replays_the_reference_reload_and_icmp_tests():
    def make(tcp, udp, dflt):
        ct = F.Conntrack(None, 4, seed=K.SEED, tcp_ns=tcp, udp_ns=udp, default_ns=dflt, max_batch=8)
        return _Ctx(R.HostTableAsModel(ct), ct.close)
    replay_golden(make)
