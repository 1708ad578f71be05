"""Restore: replaying a BackupInstruction stream over decoded bundles on the GPU.

  restore()                  -> instruction replay        backup_restorer.cc:38-107
  Bundle::Reader::Reader     -> id -> chunk map           bundle.cc:220-232
  Bundle::Reader::get        -> the chunk's bytes         bundle.cc:235-251

`Restorer.plan` is host bookkeeping: the parse (zc_parse_instructions), the id
map, which bundles the stream references and where their decoded payloads go in
one scratch buffer, and one scatter list over both the chunk extents and the
bytes_to_emit runs.  `Restorer.replay` runs that list in one zc_bundle_scatter
call, HBM to HBM.  Decoding the referenced bundles' lzo1x streams into the
scratch buffer is the caller's step between the two (liblzo2's
lzo1x_decompress_safe, as the reference calls it, compression.cc:472-490;
`bundle.frame_info` reads the frame): the instruction stream travels to the
device in the same buffer, so there is one upload (`RestorePlan.host_image`;
`RestorePlan.instruction_image` is the instruction stream's share of it alone).
"""
import numpy as np

from . import _lib
from .bundle import BundleCompressor, parse_backup_data


def chunk_map(bundles):
    """id blob -> (bundle, offset in its payload, size), as Bundle::Reader::Reader
    builds it per bundle (bundle.cc:220-232): chunks lie back to back in the
    order of the bundle's BundleInfo.  `bundles[b]` = [(chunk id blob, size), ...].
    An id twice in one bundle is an error, as there; an id in two bundles
    keeps the first."""
    out = {}
    for b, chunks in enumerate(bundles):
        pos, seen = 0, set()
        for blob, size in chunks:
            blob = bytes(blob)
            if len(blob) != 24:
                raise _lib.ZcError(f"bundle {b}: a chunk id of {len(blob)} bytes")
            if blob in seen:
                raise _lib.ZcError(f"bundle {b}: chunk id {blob.hex()} twice in one bundle")
            seen.add(blob)
            out.setdefault(blob, (b, pos, int(size)))
            pos += int(size)
    return out


class RestorePlan:
    """What one restore does: `length` bytes out; the decoded payload of bundle
    `used[k]` (`pay_size[k]` bytes) belongs at `pay_off[k]` of a scratch buffer
    of `work_size` bytes, the instruction stream `data` at `instr_off`; the
    scatter list is src_off / sizes / dst_off."""
    __slots__ = ("data", "length", "used", "pay_off", "pay_size", "instr_off", "work_size", "src_off", "sizes",
                 "dst_off")

    def host_image(self, payloads):
        """The scratch buffer's contents as one host array, for one upload:
        `payloads[k]` = the decoded payload of bundle `used[k]`."""
        img = np.zeros(max(self.work_size, 1), dtype=np.uint8)
        for k, p in enumerate(payloads):
            if len(p) != self.pay_size[k]:
                raise _lib.ZcError(f"restore: bundle {self.used[k]} decoded to {len(p)} bytes, its chunks take "
                                   f"{self.pay_size[k]}")
            img[self.pay_off[k]:self.pay_off[k] + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        img[self.instr_off:self.instr_off + len(self.data)] = np.frombuffer(self.data, dtype=np.uint8)
        return img


    def instruction_image(self):
        """(offset in the scratch buffer, the bytes that belong there): the
        instruction stream alone, whose bytes_to_emit runs the scatter list
        reads.  All of the scratch buffer that has to come from the host when
        the payloads are put at pay_off[k] on the device; host_image() is
        this plus the payloads."""
        return self.instr_off, np.frombuffer(self.data, dtype=np.uint8)


class Restorer:
    """Replays a BackupInstruction stream over decoded bundle payloads on the GPU."""

    def __init__(self, device=0, ctx=None):
        self._comp = BundleCompressor(device=device, ctx=ctx)

    @staticmethod
    def plan(backup_data, bundles):
        """Raises ZcError naming the id when the stream names a chunk no
        bundle holds (and on a malformed stream, or an id twice in a bundle)."""
        backup_data = bytes(backup_data)
        ins = parse_backup_data(backup_data)
        ids = chunk_map(bundles)
        p = RestorePlan()
        p.data = backup_data
        # the bundles the stream references, in first-use order, back to back (16-byte aligned)
        slot, p.used, p.pay_off, p.pay_size = {}, [], [], []
        pos = 0
        entries = []
        for e in ins:
            if e["kind"] == _lib.ZC_INSTR_CHUNK:
                blob = e["id"].tobytes()
                hit = ids.get(blob)
                if hit is None:
                    raise _lib.ZcError(f"restore: chunk id {blob.hex()} is in none of the {len(bundles)} bundles")
                b, off, size = hit
                if b not in slot:
                    slot[b] = len(p.used)
                    p.used.append(b)
                    p.pay_off.append(pos)
                    total = sum(int(s) for _, s in bundles[b])
                    p.pay_size.append(total)
                    pos += (total + 15) & ~15
                entries.append((p.pay_off[slot[b]] + off, size))
            else:
                entries.append((-1 - int(e["data_off"]), int(e["size"])))
        p.instr_off = pos
        p.work_size = pos + len(backup_data)
        p.src_off = np.array([s if s >= 0 else p.instr_off + (-1 - s) for s, _ in entries], dtype=np.uint64)
        p.sizes = np.array([n for _, n in entries], dtype=np.uint64)
        p.dst_off = (np.concatenate([[0], np.cumsum(p.sizes)[:-1]]).astype(np.uint64) if len(entries)
                     else np.zeros(0, dtype=np.uint64))
        p.length = int(p.sizes.sum())
        return p

    def replay(self, plan, d_work, d_out, out_cap):
        """d_work: the device copy of the plan's scratch buffer (see
        RestorePlan.host_image).  Writes the restored stream to d_out (room
        out_cap) in one scatter call and returns its length."""
        if plan.length > out_cap:
            raise _lib.ZcError(f"restore: {plan.length} bytes to restore, room for {out_cap}")
        keep = plan.sizes > 0
        if keep.any():
            self._comp.scatter(d_work, plan.src_off[keep], plan.sizes[keep], d_out, plan.dst_off[keep])
        return plan.length

    def close(self):
        self._comp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
