"""The corpus of tests/host_docs.py, proved sound without a GPU: the host codec gives every document the
stated status, the CPU oracle accepts the host-decoded records with the expected handles (specs registered
in document order), the refused spec is refused with KWOK_EDOMAIN, and every batch holds the stated
number of documents of each listing kind - where the kind a document is stated to have is the one a model
of the device's decision (json.hip k_json_pods: all_host, an escape in a compared string, the spec table
keyed by kwok_spec_key) gives for the specs registered when the call starts."""
from collections import Counter

import pytest

import host_docs as hd
from kwok_amd import abi
from kwok_amd.engine import KwokError, make_config, spec_key
from oracle.oracle import Oracle


def build(name, monkeypatch):
    sc = hd.SCENARIOS[name]()
    if sc.key_bits:
        monkeypatch.setenv("KWOK_DEBUG_SPEC_KEY_BITS", str(sc.key_bits))
    return sc


def listing(sc, registered, l):
    """the kind k_json_pods gives the line when `registered` is the spec table of the call"""
    if sc.codec_kw is hd.NINE or l.esc:
        return "host"
    if l.type == "DELETED":
        return "dev"  # (the spec of a Deleted line's object is not looked up)
    bits = sc.key_bits or 64
    key = hd.fnv_key(l.spec, bits)
    holders = [s for s in registered if hd.fnv_key(s, bits) == key]
    if key == 0 or len(holders) != 1:  # (key 0 marks an empty slot; a key two specs share answers -2)
        return "spec2" if l.spec in registered else "spec"
    return "dev" if holders[0] == l.spec else "specx"


@pytest.mark.parametrize("name", list(hd.SCENARIOS))
def test_corpus_against_the_host_codec_and_the_oracle(name, monkeypatch):
    sc = build(name, monkeypatch)
    ref = hd.Ref(sc)
    now = hd.T0
    seen = list(sc.pre_specs)
    for b in sc.batches:
        where = "%s / %s" % (name, b.name)
        registered = list(ref.spec_id)
        got = Counter(l.kind for l in b.lines)
        assert got == Counter({k: v for k, v in b.kinds.items() if v}), where
        for k, l in enumerate(b.lines):
            assert l.kind == listing(sc, registered, l), "%s #%d" % (where, k)
            if l.type != "DELETED":
                c, i, g = l.spec
                assert spec_key(list(c), list(i), list(g)) == hd.fnv_key(l.spec, sc.key_bits or 64), "%s #%d" % (where, k)
        # n_host: the JSON_HOST documents, every other upsert whose spec is not registered when the call
        # starts, the JSON_SPEC_X documents (and, under cut keys, the upserts whose key the table does not answer)
        unregistered = sum(1 for l in b.lines if l.kind != "host" and l.type != "DELETED" and l.spec not in registered
                           and l.kind != "specx")
        assert b.n_host == got["host"] + unregistered + got["specx"] + got["spec2"] > 0, where
        assert unregistered == got["spec"], where
        live = set(ref.by_uid.values())
        sent, hs, st, rel, decoded = ref.expect(b)
        for k, l in enumerate(b.lines):
            at = "%s #%d" % (where, k)
            assert decoded[k] == (abi.OK if l.refused else l.status), at   # Codec.decode_pods(strict=False)
            assert st[k] == l.status, at
            if l.status != abi.OK:
                assert hs[k] == -1 and rel[k] == 0, at
            elif sent[k] >= 0:
                assert hs[k] == sent[k], at
            else:
                assert l.type == "ADDED" and hs[k] >= 0 and hs[k] not in live, at
                live.add(int(hs[k]))
            if l.type != "DELETED" and l.status == abi.OK and l.spec not in seen:
                seen.append(l.spec)
            if l.type == "DELETED" and l.status == abi.OK and sent[k] >= 0 and b"podIP" in l.doc:
                assert rel[k] != 0, at  # (a pod that held an address of the CIDR gives it back)
        # the oracle's ids are the first-appearance order of the documents
        assert list(ref.spec_id) == seen and list(ref.spec_id.values()) == list(range(len(seen))), where
        ref.o.tick(now)
        now += 30
    for s in sc.unseen:
        assert s not in ref.spec_id
    assert sum(len(b.lines) for b in sc.batches) >= 9
    ref.close()


def test_listed_counts_cross_the_block_edge():
    sc = hd.SCENARIOS["block-edges"]()
    assert [b.n_host for b in sc.batches] == [1, 2, 255, 256, 257]
    assert all(b.create_only for b in sc.batches)


def test_collision_scenario_holds_a_spec_x_ahead_of_the_rest():
    sc = hd.SCENARIOS["spec-collisions"]()
    kinds = [l.kind for l in sc.batches[1].lines]
    assert kinds[0] == "specx" and kinds.index("specx") < kinds.index("spec") < kinds.index("host")
    specs = {l.spec for l in sc.batches[1].lines} - {l.spec for l in sc.batches[0].lines}
    assert len(specs) == 3
    assert all(sum(1 for l in sc.batches[1].lines if l.spec == s) == 2 for s in specs)


def test_the_refused_spec_is_refused_by_the_oracle():
    """a patch longer than 64 KiB: kwok_register_pod_spec answers KWOK_EDOMAIN, and nothing else does"""
    o = Oracle(make_config(**hd.KW))
    c, i, g = hd.BIG
    assert len(c) == 32 and sum(len(n) + len(im) for n, im in c) > 0xFFF0
    with pytest.raises(KwokError) as ei:
        o.register_pod_spec(list(c), list(i), list(g))
    assert ei.value.code == abi.EDOMAIN
    assert o.register_pod_spec(list(hd.A[0]), [], []) == 0  # (the refusal took no id)
    o.close()
    sc = hd.SCENARIOS["refused-spec"]()
    lines = sc.batches[0].lines
    bad = [k for k, l in enumerate(lines) if l.status != abi.OK]
    assert len(bad) == 1 and lines[bad[0]].refused and lines[bad[0]].status == abi.EDOMAIN
    assert any(l.kind != "dev" for l in lines[:bad[0]]) and any(l.kind != "dev" for l in lines[bad[0] + 1:])
