#!/usr/bin/env python3
"""Write tests/golden/dns_capture_expect.json: what every UDP DNS message of
tests/golden/test_dns.pcap holds, parsed by dnspython (an implementation that
shares nothing with this project or its model): per frame the ID and, in
message order, (section, owner name, type, class, TTL) of every question and
resource record. Needs dnspython; the tests read the file only.

    python tools/make_dns_capture_expect.py

dnspython lifts the OPT record out of the additional section; it is put back
where the wire has it, with the class and TTL its fields make up (RFC 6891
6.1.2-6.1.3: class = payload size, TTL = extended RCODE, version, flags).
"""
import json
import os
import struct
import sys

import dns.message
import dns.rdatatype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import pktutil
    frames = [f for f in pktutil.read_pcap(os.path.join(pktutil.GOLDEN, "test_dns.pcap"))[1]
              if len(f) > 42 and f[12:14] == b"\x08\x00" and f[23] == 17 and 53 in struct.unpack(">HH", f[34:38])]
    out = []
    for k, f in enumerate(frames):
        m = dns.message.from_wire(f[42:], one_rr_per_rrset=True)
        rows = []
        for q in m.question:
            rows.append([0, q.name.to_text(omit_final_dot=True), int(q.rdtype), int(q.rdclass), 0])
        for sec, rrsets in ((1, m.answer), (2, m.authority), (3, m.additional)):
            for rs in rrsets:
                rows.append([sec, rs.name.to_text(omit_final_dot=True), int(rs.rdtype), int(rs.rdclass), int(rs.ttl)])
        if m.opt is not None:  # the captures carry it as the last additional record
            assert f[42 + 10:42 + 12] != b"\x00\x00" and not m.additional
            rows.append([3, "", int(dns.rdatatype.OPT), int(m.payload), int(m.ednsflags)])
        for r in rows:
            r[1] = "" if r[1] == "@" else r[1]
        out.append(dict(frame=k, frame_bytes=len(f), id=m.id, entries=rows))
    path = os.path.join(ROOT, "tests", "golden", "dns_capture_expect.json")
    with open(path, "w") as fh:
        json.dump(dict(source="tests/golden/test_dns.pcap", parser="dnspython", frames=out), fh, indent=1)
        fh.write("\n")
    print("%d frames -> %s" % (len(out), path))


if __name__ == "__main__":
    main()
