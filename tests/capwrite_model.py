"""A plain-Python restatement of the reference's capture writers, the checker
of the capwrite tests: pcapgo.Writer (pcapgo/write.go:25-129) and
pcapgo.NgWriter (ngwrite.go:45-416, ngwrite_dsb.go:71-110). A sequence of
calls becomes the bytes the reference hands its io.Writer. Times are (Unix
seconds, nanoseconds) pairs; the zero time.Time is ZERO. Strings are bytes.

It is pinned two ways: the reference's own byte vectors
(tests/golden/capwrite_vectors.json, from write_test.go) and round trips of
the reference's writer tests through the project's reader, which the reader
oracle pins in turn (test_capwrite_cpu.py).

frame_batch() is the batch contract of include/gpk_capwrite.h stated with
these writers: one WritePacket per output packet, errors and overflow as the
header defines them."""
import struct

ZERO = (-62135596800, 0)
NO_VALUE64 = (1 << 64) - 1
PCAP_MICRO, PCAP_NANO, PCAPNG = 1, 2, 3
OK, ELENGTH, EIFACE, EBIG, EINDEX = 0, -32, -33, -34, -35
SECRET_TYPES = (0x5353484b, 0x5a4e574b, 0x57474b4c, 0x5a415053, 0x544c534b)
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


class WriteError(Exception):
    pass


def unix_nano(t):
    """Time.UnixNano(): int64 arithmetic that wraps."""
    return (t[0] * 1000000000 + t[1]) & M64


def u32(v):
    return struct.pack("<I", v & M32)


def pad4(n):
    return (4 - (n & 3)) & 3


def ng_options(options):
    """prepareNgOptions + writeOptions: [(code, kind, value)], kind in
    bytes/time/u64/u32/u8."""
    if not options:
        return b""
    out = b""
    for code, kind, v in options:
        if kind == "bytes":
            body = bytes(v) + bytes(pad4(len(v)))
            n = len(v)
        elif kind == "time":
            ts = unix_nano(v)
            body, n = u32(ts >> 32) + u32(ts), 8
        elif kind == "u64":
            body, n = struct.pack("<Q", v), 8
        elif kind == "u32":
            body, n = u32(v), 4
        else:  # uint8, written as 4 bytes
            body, n = bytes([v, 0, 0, 0]), 1
        out += struct.pack("<HH", code, n & 0xFFFF) + body
    return out + bytes(4)


def packet_options(o):
    """NgPacketOptions.toNgOptions (pcapng.go:352-410); o is a dict with the
    struct's member names, absent or None members unset."""
    if not o:
        return []
    out = [(1, "bytes", c) for c in o.get("Comments") or []]
    if o.get("Flags") is not None:
        out.append((2, "u32", o["Flags"]))
    out += [(3, "bytes", bytes([a]) + bytes(h)) for a, h in o.get("Hashes") or []]
    if o.get("DropCount") is not None:
        out.append((4, "u64", o["DropCount"]))
    if o.get("PacketID") is not None:
        out.append((5, "u64", o["PacketID"]))
    if o.get("Queue") is not None:
        out.append((6, "u32", o["Queue"]))
    out += [(7, "bytes", bytes([t]) + bytes(d)) for t, d in o.get("Verdicts") or []]
    return out


class PcapWriter:
    def __init__(self, nanos=False, now=(0, 0)):
        self.scaler = 1 if nanos else 1000
        self.now = now  # what time.Now() returns
        self.out = bytearray()

    def write_file_header(self, snaplen, linktype):
        magic = 0xA1B2C3D4 if self.scaler == 1000 else 0xA1B23C4D
        self.out += struct.pack("<IHHIIII", magic, 2, 4, 0, 0, snaplen & M32, linktype & M32)

    def write_packet(self, ts, caplen, length, data):
        if caplen != len(data):
            raise WriteError("capture length %d does not match data length %d" % (caplen, len(data)))
        if caplen > length:
            raise WriteError("capture length > length")
        ts = (ts[0] + ts[1] // 1000000000, ts[1] % 1000000000)  # time.Unix normalises
        if ts == ZERO:
            ts = self.now
        self.out += u32(ts[0]) + u32(ts[1] // self.scaler) + u32(caplen) + u32(length) + bytes(data)


class NgWriter:
    def __init__(self, intf, section):
        """NewNgWriterInterface: section = dict(Application, Comment, Hardware, OS)."""
        self.out = bytearray()
        self.intf = 0
        opts = [(code, "bytes", section[k]) for code, k in ((4, "Application"), (1, "Comment"), (2, "Hardware"),
                                                            (3, "OS")) if section.get(k)]
        body = ng_options(opts)
        length = len(body) + 24 + 4
        self.out += struct.pack("<IIIHHQ", 0x0A0D0D0A, length, 0x1A2B3C4D, 1, 0, M64) + body + u32(length)
        self.add_interface(intf)

    def add_interface(self, f):
        """f = dict(Name, Comment, Description, Filter, OS, LinkType, TimestampOffset, SnapLength)."""
        ident = self.intf
        self.intf += 1
        opts = []
        if f.get("Name"):
            opts.append((2, "bytes", f["Name"]))
        if f.get("Comment"):
            opts.append((1, "bytes", f["Comment"]))
        if f.get("Description"):
            opts.append((3, "bytes", f["Description"]))
        if f.get("Filter"):
            opts.append((11, "bytes", b"\x00" + f["Filter"]))
        if f.get("OS"):
            opts.append((12, "bytes", f["OS"]))
        if f.get("TimestampOffset"):
            opts.append((14, "u64", f["TimestampOffset"]))
        opts.append((9, "u8", 9))
        body = ng_options(opts)
        length = len(body) + 16 + 4
        self.out += struct.pack("<IIHHI", 1, length, f.get("LinkType", 0) & 0xFFFF, 0,
                                f.get("SnapLength", 0) & M32) + body + u32(length)
        return ident

    def write_interface_stats(self, intf, s):
        """s = dict(LastUpdate, StartTime, EndTime, PacketsReceived, PacketsDropped)."""
        if intf >= self.intf or intf < 0:
            raise WriteError("Can't send statistics for non existent interface %d; have only %d interfaces"
                             % (intf, self.intf))
        opts = []
        if s.get("StartTime", ZERO) != ZERO:
            opts.append((2, "time", s["StartTime"]))
        if s.get("EndTime", ZERO) != ZERO:
            opts.append((3, "time", s["EndTime"]))
        if s.get("PacketsDropped", NO_VALUE64) != NO_VALUE64:
            opts.append((5, "u64", s["PacketsDropped"]))
        if s.get("PacketsReceived", NO_VALUE64) != NO_VALUE64:
            opts.append((4, "u64", s["PacketsReceived"]))
        body = ng_options(opts)
        length = len(body) + 24
        lu = s.get("LastUpdate", ZERO)
        ts = 0 if lu == ZERO else unix_nano(lu)
        self.out += struct.pack("<III", 5, length, intf) + u32(ts >> 32) + u32(ts) + body + u32(length)

    def write_packet(self, ts, caplen, length, iface, data, options=None):
        if iface >= self.intf or iface < 0:
            raise WriteError("Can't send statistics for non existent interface %d; have only %d interfaces"
                             % (iface, self.intf))
        if caplen != len(data):
            raise WriteError("capture length %d does not match data length %d" % (caplen, len(data)))
        if caplen > length:
            raise WriteError("capture length > length")
        body = ng_options(packet_options(options))
        total = len(body) + 28 + len(data) + 4
        padding = pad4(total)
        total += padding
        t = unix_nano(ts)
        self.out += (struct.pack("<III", 6, total & M32, iface & M32) + u32(t >> 32) + u32(t) + u32(caplen)
                     + u32(length) + bytes(data) + bytes(padding) + body + u32(total))

    def write_secrets(self, typ, payload):
        if typ not in SECRET_TYPES:
            raise WriteError("Unknown Decryption Secrets Block (DSB) type")
        padding = pad4(len(payload))
        length = 8 + 4 + 8 + len(payload) + padding
        self.out += struct.pack("<IIII", 10, length, typ, len(payload)) + bytes(payload) + bytes(padding) + u32(length)


def frame_batch(fmt, interfaces, packets, ci, order=None, options=None, now=(0, 0), out_cap=None):
    """include/gpk_capwrite.h's batch contract over the writers above.
    packets: list of bytes; ci: list of (ts_sec, ts_nsec, length, iface);
    options: per OUTPUT packet, already encoded bytes (or None). Returns
    (blocks: list of bytes, b"" for a packet in error; block_off; status;
    counts) with the blocks that do not end inside out_cap still listed (the
    caller cuts them)."""
    order = list(range(len(packets))) if order is None else list(order)
    blocks, status = [], []
    for j, i in enumerate(order):
        opt = (options[j] if options is not None else None) or b""
        if not 0 <= i < len(packets):
            blocks.append(b"")
            status.append(EINDEX)
            continue
        sec, nsec, length, iface = ci[i]
        data = packets[i]
        if fmt == PCAPNG:
            w = NgWriter.__new__(NgWriter)
            w.out, w.intf = bytearray(), interfaces
            if iface >= interfaces or iface < 0:
                st = EIFACE
            elif len(data) > length:
                st = ELENGTH
            elif 28 + len(data) + pad4(len(data)) + len(opt) + 4 >= 1 << 32:
                st = EBIG
            else:
                st = OK
                w.write_packet((sec, nsec), len(data), length, iface, data)
                w.out[-4:-4] = opt  # the encoded options sit between the padding and the trailing length
                total = len(w.out)
                w.out[4:8] = u32(total)
                w.out[-4:] = u32(total)
        else:
            w = PcapWriter(nanos=fmt == PCAP_NANO, now=now)
            st = ELENGTH if len(data) > length else OK
            if st == OK:
                w.write_packet((sec, nsec), len(data), length, data)
        blocks.append(bytes(w.out) if st == OK else b"")
        status.append(st)
    off = [0]
    for b in blocks:
        off.append(off[-1] + len(b))
    cap = off[-1] if out_cap is None else out_cap
    written = sum(1 for j, b in enumerate(blocks) if b and off[j + 1] <= cap)
    counts = [written, off[-1], sum(1 for s in status if s != OK), int(off[-1] > cap)]
    return blocks, off, status, counts
