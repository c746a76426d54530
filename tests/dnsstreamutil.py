"""Helpers shared by the DNS-over-streams tests (CPU and GPU)."""
import numpy as np

import configs
import dnsstream_model as SM
from gopacket_amd import flows

KEYS = flows.DNSStreamDecoder.KEYS
ARENAS = ("msgs", "rrs", "names", "tails")


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
    """gpk_dns_streams_host over the calls of a dnsstream_model.Streaming: the
    reassembly comes from the model, state and tails are chained from the host
    entry's own outputs, per global stream id."""

    def __init__(self, cfg, frame_unstarted=False, max_message=0):
        self.parser = configs.device_parser(cfg)
        self.frame_unstarted, self.max_message = frame_unstarted, max_message
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
        hcaps = [len(m[k]) for k in ARENAS]
        h = flows.DNSStreamDecoder.decode_host(self.parser, data, off, cap, ref["records"], ref["layouts"], asm, *hcaps,
                                               carry=self.carry(last["ids"]), frame_unstarted=self.frame_unstarted,
                                               max_message=self.max_message, fill=fill)
        if keep:
            for j, (g, st) in enumerate(zip(last["ids"], last["asm"]["streams"])):
                e = h["streams"][j]
                if st["closed"] != SM.AM.OPEN:
                    self.state.pop(g, None)
                else:
                    self.state[g] = (int(e["state"]), int(e["tail_off"]), int(e["tail_len"]))
            self.tails = h["tails"]
        return m, h


def steps_of(case):
    return [(pk, False) for pk in case["calls"]] + ([([], True)] if case["flush"] else [])


def run_case_host(case, on_call=None):
    """A case of dnsstreamcases through the model and the host entry; returns
    the model's per-call results. on_call(model.last): for a recorder."""
    cfg = case["parser"]
    model = SM.Streaming(cfg, case["max_pages"], case["frame_unstarted"], case["max_message"])
    chain = HostChain(cfg, case["frame_unstarted"], case["max_message"])
    calls = []
    for k, (pk, flush) in enumerate(steps_of(case)):
        res = model.feed(pk, flush=flush)
        calls.append(res)
        if model.last is None:
            continue
        if on_call:
            on_call(model.last)
        m, h = chain.call(model.last)
        assert_same_streams(m, h, "%s call %d" % (case["name"], k))
    return calls


def mix_case(calls, **kw):
    import dnsstreamcases as SC
    return dict(dict(name="mix", calls=calls, max_pages=0, frame_unstarted=False, flush=True, max_message=0,
                     parser=SC.PARSER), **kw)
