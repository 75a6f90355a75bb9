"""tests/strgraph_reference.py against the reference: every call recorded in
tests/golden/golden_assembly.json -- the reference's list and its shuffled
order, default options, cutoffs of 1 and a raised -l -- gives X.contigs.fas with
the recorded md5 and the recorded stdout, byte for byte.  And every rule the
restatement names changes some golden or generated result when it is broken."""
import hashlib

import numpy as np
import pytest

import assembly_golden as ag
import strgraph_reference as sg


def test_the_sets_are_the_six_of_the_issue():
    assert sorted(ag.GOLDEN) == ["circ", "inv", "none", "rep2", "rep3", "var"]
    assert ag.GOLDEN["none"]["matches"] == 0
    shown = {n: ag.GOLDEN[n]["calls"]["d1l1"]["stdout"] for n in ag.GOLDEN}
    assert "no contigs respect" in shown["none"] and "number of contigs:     1\n" in shown["circ"]
    # the order of the list decides some outputs: the shuffled lists pin the insertion-order rule
    assert any(ag.GOLDEN[n]["shuffled"]["default"]["md5"] != ag.GOLDEN[n]["calls"]["default"]["md5"] for n in ag.GOLDEN)


@pytest.mark.parametrize("name,which,key", ag.CALLS)
def test_every_golden_call(name, which, key):
    reads, records, want = ag.call(name, which, key)
    found = sg.contigs(reads, records, *ag.options(name, key))
    raw = sg.fasta(found)
    assert (hashlib.md5(raw).hexdigest(), len(raw)) == (want["md5"], want["size"])
    assert sg.stdout(reads, found).decode() == want["stdout"]


def test_shapes_of_the_goldens():
    """what the sets were made to show"""
    def paths(name, which="calls", key="d1l1"):
        reads, records, _ = ag.call(name, which, key)
        return [(sg.vertex_name(c[2]), sg.vertex_name(c[3]), c[1]) for c in sg.contigs(reads, records, *ag.options(name, key))]
    circ = paths("circ")
    assert len(circ) == 1 and circ[0][0] == circ[0][1] and circ[0][2] == 51
    assert any(a[:-1] == b[:-1] and a[-1] != b[-1] for a, b, _ in paths("inv"))          # a hairpin
    firsts = [a for a, _, _ in paths("rep3")]
    assert max(firsts.count(a) for a in firsts) >= 2                                      # a junction starts several
    reads, records, _ = ag.call("rep3", "calls", "d1l1")
    adj = sg.build_graph([len(r) for r in reads], records)
    assert max(len(e) for e in adj) >= 3


@pytest.mark.parametrize("rule", sg.RULES)
def test_every_rule_is_pinned(rule):
    """a restatement with one rule broken misses a golden call or a generated shape"""
    assert ag.first_miss(rule) is not None, rule


def test_multiset_of_contigs_does_not_depend_on_list_order():
    """what the end-to-end comparison of the command-line test rests on: at the
    default cutoffs the contigs as a multiset of min(sequence, reverse complement)
    are those of the reference's list whatever the order of the list"""
    for name in ag.E2E_SETS:
        reads, records, _ = ag.call(name, "calls", "default")
        want = sg.canonical(sg.contigs(reads, records))
        reads, shuffled, _ = ag.call(name, "shuffled", "default")
        assert sg.canonical(sg.contigs(reads, shuffled)) == want, name
        rng = np.random.default_rng(5)
        for _ in range(5):
            assert sg.canonical(sg.contigs(reads, records[rng.permutation(records.shape[0])])) == want, name


def test_the_reference_s_seconds_on_the_probe_s_set_name_their_cpu():
    """tests/golden/golden_assembly_probe.json, what DESIGN.md sets beside the device times"""
    import json
    import os
    with open(os.path.join(ag.ou.GOLDEN_DIR, "golden_assembly_probe.json")) as f:
        probe = json.load(f)
    assert sorted(probe["seconds"]) == ["assembly", "overlap", "prefilter"] and all(v > 0 for v in probe["seconds"].values())
    assert probe["cpu"]["model name"] and probe["cpu"]["model"] and probe["reads"] > 300000 and probe["matches"] > 300000
    assert probe["contigs"]["stdout"].startswith("# gt readjoiner assembly") and len(probe["contigs"]["md5"]) == 32
