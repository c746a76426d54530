"""Helpers shared by the TLS-over-streams tests (CPU and GPU)."""
import numpy as np

import configs
import tlsstream_model as SM
from gopacket_amd import flows

KEYS = flows.TLSStreamDecoder.KEYS


def assert_same_streams(m, h, what=""):
    """Every output array byte for byte (what lies past counts[0] and past the
    capacities' use included: it keeps the fill)."""
    for k in KEYS:
        a, b = np.asarray(m[k]), np.asarray(h[k])
        assert a.size == b.size, (what, k, a.size, b.size)
        if a.dtype.fields:
            bad = [j for j in range(len(a)) if a[j].tobytes() != b[j].tobytes()]
            assert not bad, "%s: %s differ at entries %s: model %s got %s" % (what, k, bad[:5], a[bad[:2]], b[bad[:2]])
        else:
            assert np.array_equal(a.astype(np.uint64), b.astype(np.uint64)), "%s: %s differs: model %s got %s" % (
                what, k, a[:16], b[:16])


class HostChain:
    """gpk_tls_streams_host over the calls of a tlsstream_model.Streaming: the
    reassembly comes from the model, state and tails are chained from the host
    entry's own outputs, per global stream id."""

    def __init__(self, cfg, frame_unstarted=False):
        self.parser = configs.device_parser(cfg)
        self.frame_unstarted = frame_unstarted
        self.state, self.tails = {}, np.zeros(0, np.uint8)

    def carry(self, ids):
        st = np.array([self.state.get(g, (SM.NEW, 0, 0)) for g in ids], np.int64).reshape(len(ids), 3)
        return (st[:, 0].astype(np.uint32), st[:, 1].astype(np.uint64), st[:, 2].astype(np.uint32), self.tails)

    def call(self, last, caps=(None,) * 4, fill=0xA5, keep=True):
        """(model arrays, host arrays) of the call the model made last."""
        data, off, cap, ref = last["arrays"]
        n = len(cap)
        asm = SM.asm_arrays(last["asm"], n)
        m = SM.to_arrays(last["res"], n, caps, fill)
        hcaps = [len(m[k]) for k in ("recs", "hellos", "snis", "tails")]
        h = flows.TLSStreamDecoder.decode_host(self.parser, data, off, cap, ref["records"], ref["layouts"], asm, *hcaps,
                                               carry=self.carry(last["ids"]), frame_unstarted=self.frame_unstarted,
                                               fill=fill)
        if keep:
            for j, (g, st) in enumerate(zip(last["ids"], last["asm"]["streams"])):
                e = h["streams"][j]
                if st["closed"] != SM.AM.OPEN:
                    self.state.pop(g, None)
                else:
                    self.state[g] = (int(e["state"]), int(e["tail_off"]), int(e["tail_len"]))
            self.tails = h["tails"]
        return m, h


def run_case_host(case, cfg):
    """A case of tlsstreamcases through the model and the host entry; returns
    the model's per-call results."""
    model = SM.Streaming(cfg, case["max_pages"], case["frame_unstarted"])
    chain = HostChain(cfg, case["frame_unstarted"])
    calls = []
    steps = [(pk, False) for pk in case["calls"]] + ([([], True)] if case["flush"] else [])
    for k, (pk, flush) in enumerate(steps):
        res = model.feed(pk, flush=flush)
        calls.append(res)
        if model.last is None:
            continue
        m, h = chain.call(model.last)
        assert_same_streams(m, h, "%s call %d" % (case["name"], k))
    return calls


def names_of(res):
    """[(global id, server name)] of a model call result."""
    return [(d["id"], e["client_hello"]["sni"]) for d in res for e in d["entries"]
            if "client_hello" in e and e["client_hello"]["has_sni"]]
