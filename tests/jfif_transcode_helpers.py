"""Marker surgery shared by the transcoder's tests: a JPEG file's component ids rewritten in its frame header and in every scan header,
and the ids read back -- an independent walk over every marker SOI .. EOI (entropy-coded data is skipped byte by byte)."""


def _walk(data):
    """yields (marker, start, end) of every marker segment of a whole file, scans' SOS included"""
    i, n = 2, len(data)
    while i + 4 <= n:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xD9:
            return
        length = (data[i + 2] << 8) | data[i + 3]
        yield m, i, i + 2 + length
        i += 2 + length
        if m == 0xDA:                                # entropy-coded data: up to the next marker that is not a stuffed byte or RSTn
            while not (data[i] == 0xFF and data[i + 1] != 0x00 and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1


def with_ids(data, ids):
    """the file with its three component ids replaced by `ids`, in SOF0 / SOF1 / SOF2 and in every SOS"""
    out = bytearray(data)
    old = None
    for m, a, b in _walk(data):
        if m in (0xC0, 0xC1, 0xC2):
            assert data[a + 9] == 3
            old = [data[a + 10 + 3 * k] for k in range(3)]
            for k in range(3):
                out[a + 10 + 3 * k] = ids[k]
        elif m == 0xDA:
            for c in range(data[a + 4]):
                out[a + 5 + 2 * c] = ids[old.index(data[a + 5 + 2 * c])]
    return bytes(out)


def ids_of(data):
    """-> (frame ids, [ids of each scan])"""
    frame, scans = None, []
    for m, a, b in _walk(data):
        if m in (0xC0, 0xC1, 0xC2):
            frame = [data[a + 10 + 3 * k] for k in range(data[a + 9])]
        elif m == 0xDA:
            scans.append([data[a + 5 + 2 * c] for c in range(data[a + 4])])
    return frame, scans
