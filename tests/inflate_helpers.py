"""What the GPU tests of csrc/inflate.hip share: one guarded aej_inflate_batch launch, a bit writer for hand-made streams, the zlib header
and the .ajpg container writer."""
import ctypes
import zlib

import numpy as np

GUARD = 0xA5


def run_inflate(A, ctx, streams, caps=None, fill=0):
    """-> (outputs, statuses, guards intact) for streams decoded in ONE aej_inflate_batch launch into a guarded buffer.  fill: the byte
    between the streams in the source buffer (a stream ends up to three bytes before the next one starts, and the last one before the
    buffer does)."""
    import torch
    n = len(streams)
    in_off, pos = [], 0
    for s in streams:
        in_off.append(pos)
        pos += (len(s) + 3) // 4 * 4
    src = np.full(max(pos, 4), fill, np.uint8)
    for o, s in zip(in_off, streams):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    caps = caps or [len(zlib.decompress(s)) if ok else 1 << 16 for s, ok in zip(streams, [True] * n)]
    out_off, pos = [], 0
    for c in caps:
        out_off.append(pos)
        pos += (c + 3) // 4 * 4 + 256              # guard bytes after every slot
    dst = torch.full((pos,), GUARD, dtype=torch.uint8, device="cuda")
    desc = np.array([[in_off[i], len(streams[i]), out_off[i], caps[i]] for i in range(n)], np.int64)
    d_src, d_desc = torch.from_numpy(src).cuda(), torch.from_numpy(desc).cuda()
    out_bytes = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.aej_inflate_batch(ctx.handle, d_src.data_ptr(), d_desc.data_ptr(), n, dst.data_ptr(), ctypes.c_uint64(pos),
                                        out_bytes.data_ptr(), status.data_ptr()))
    host = dst.cpu().numpy()
    nb, st = out_bytes.cpu().numpy(), status.cpu().numpy()
    outs, guards = [], True
    for i in range(n):
        outs.append(host[out_off[i]:out_off[i] + nb[i]].tobytes())
        end = out_off[i] + nb[i] if st[i] == 0 else out_off[i] + caps[i]
        nxt = out_off[i + 1] if i + 1 < n else pos
        guards &= bool(np.all(host[max(end, out_off[i] + caps[i]):nxt] == GUARD))
        if st[i] == 0:
            guards &= bool(np.all(host[end:out_off[i] + caps[i]] == GUARD))
    return outs, st, guards


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):                 # LSB first
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):                # Huffman codes MSB first
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + j] << j for j in range(8)) for i in range(0, len(b), 8))


def zhdr(cmf=0x78, fdict=0):
    flg = fdict << 5
    flg |= (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg])


def rebuild(meta_bytes, layers):
    out = [meta_bytes]
    for bits_len, root, packed, stream in layers:
        out += [bits_len.to_bytes(4, "big"), root.to_bytes(4, "big"), packed, len(stream).to_bytes(4, "big"), stream]
    return b"".join(out)
