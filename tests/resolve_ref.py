"""The resident chunk index and the resolve of a backup against it, restated in
plain Python from the reference (test infrastructure only; not derived from
zbackup_amd.restore.chunk_map and not from the code under test):

* ChunkIndex::loadIndex (chunk_index.cc:26-79) walks the bundles in input
  order and each bundle's records from the last to the first (line 55);
  registerNewChunkId (chunk_index.cc:163-182) keeps the first registration of
  an id, so findChunk (chunk_index.cc:119-161) answers with that bundle and
  that record's size;
* Bundle::Reader's map (bundle.cc:220-232): a bundle's chunks lie back to back
  in BundleInfo order, and an id met twice in one bundle is exDuplicateChunks
  (lines 229-230) -- the bundle cannot be opened;
* the resolve of a BackupInstruction stream (backup_restorer.cc:38-107 over
  ChunkStorage::Reader::get, chunk_storage.cc:214-260): used bundles ascending
  by bundle number, slot k the k-th of them, slot n_used the instruction
  stream, dst the exclusive running sum of the entry sizes.

bundles = [[(chunk id blob, size), ...], ...] in input order.  entries =
[("chunk", id blob) | ("bytes", data_off, size), ...].
"""
NO_BUNDLE = 0xFFFFFFFF
CHUNK, BYTES = 0, 1


def build(bundles):
    """{"owner": id -> (bundle, record in the bundle), "off": per bundle the
    payload offset of every record, "bundle_size": [...], "dup": [...]}"""
    owner = {}
    for b, recs in enumerate(bundles):          # loadIndex: bundles in input order
        for x in range(len(recs) - 1, -1, -1):  # for ( int x = info.chunk_record_size(); x--; )
            blob = bytes(recs[x][0])
            if blob not in owner:               # registerNewChunkId: the entry existed already
                owner[blob] = (b, x)
    off, bundle_size, dup = [], [], []
    for recs in bundles:                        # Bundle::Reader: populate the map
        chunks, nxt, offs, twice = set(), 0, [], False
        for blob, size in recs:
            if bytes(blob) in chunks:
                twice = True                    # exDuplicateChunks
            chunks.add(bytes(blob))
            offs.append(nxt)
            nxt += int(size)
        off.append(offs)
        bundle_size.append(nxt)
        dup.append(twice)
    return {"owner": owner, "off": off, "bundle_size": bundle_size, "dup": dup, "bundles": bundles}


def lookup(ix, blob):
    """findChunk, then where the owner record lies: (bundle, off, size), or
    (NO_BUNDLE, 0, 0)."""
    hit = ix["owner"].get(bytes(blob))
    if hit is None:
        return NO_BUNDLE, 0, 0
    b, x = hit
    return b, ix["off"][b][x], int(ix["bundles"][b][x][1])


def counts(ix):
    return {"records": sum(len(r) for r in ix["bundles"]), "bundles": len(ix["bundles"]),
            "ids": len(ix["owner"]), "flagged": sum(ix["dup"])}


def resolve(ix, entries):
    """The plan of zc_restore_resolve as lists."""
    hits = []
    for e in entries:
        if e[0] == "chunk":
            hits.append((CHUNK,) + lookup(ix, e[1]))
        else:
            hits.append((BYTES, None, int(e[1]), int(e[2])))
    used = sorted({b for k, b, _, _ in hits if k == CHUNK and b != NO_BUNDLE})
    slot_of = {b: k for k, b in enumerate(used)}
    out = {"used": used, "used_size": [ix["bundle_size"][b] for b in used], "slot": [], "off": [], "size": [],
           "dst": []}
    pos = 0
    missing, dups = [], []
    for i, (k, b, off, size) in enumerate(hits):
        if k == BYTES:
            out["slot"].append(len(used))
        elif b == NO_BUNDLE:
            out["slot"].append(NO_BUNDLE)
            missing.append(i)
        else:
            out["slot"].append(slot_of[b])
            if ix["dup"][b]:
                dups.append(i)
        out["off"].append(off)
        out["size"].append(size)
        out["dst"].append(pos)
        pos += size
    out.update(n_entries=len(entries), n_used=len(used), length=pos, n_missing=len(missing),
               first_missing=missing[0] if missing else 0, n_dup_used=len(dups), first_dup=dups[0] if dups else 0)
    return out


def restore_bytes(ix, entries, payloads, data):
    """The restored stream: payloads[b] = bundle b's decoded payload, data the
    instruction stream the BYTES entries point into.  Raises KeyError on a
    missing id and ValueError when a used bundle cannot be opened."""
    out = bytearray()
    for e in entries:
        if e[0] == "chunk":
            b, off, size = lookup(ix, e[1])
            if b == NO_BUNDLE:
                raise KeyError(bytes(e[1]).hex())  # exNoSuchChunk
            if ix["dup"][b]:
                raise ValueError(f"bundle {b}: exDuplicateChunks")
            out += payloads[b][off:off + size]
        else:
            out += data[e[1]:e[1] + e[2]]
    return bytes(out)


def _self_check():
    a, b, c = bytes([1]) * 24, bytes([2]) * 24, bytes([3]) * 24
    ix = build([[(a, 5), (b, 7)], [], [(b, 7), (c, 0), (c, 0)], [(a, 5)]])
    assert lookup(ix, a) == (0, 0, 5) and lookup(ix, b) == (0, 5, 7)
    assert lookup(ix, c) == (2, 7, 0)  # the last record is the first registration
    assert lookup(ix, bytes(24)) == (NO_BUNDLE, 0, 0)
    assert ix["dup"] == [False, False, True, False] and ix["bundle_size"] == [12, 0, 7, 5]
    assert counts(ix) == {"records": 6, "bundles": 4, "ids": 3, "flagged": 1}
    r = resolve(ix, [("chunk", b), ("bytes", 3, 4), ("chunk", bytes(24)), ("chunk", c), ("chunk", a)])
    assert r["used"] == [0, 2] and r["slot"] == [0, 2, NO_BUNDLE, 1, 0]
    assert r["dst"] == [0, 7, 11, 11, 11] and r["length"] == 16
    assert (r["n_missing"], r["first_missing"], r["n_dup_used"], r["first_dup"]) == (1, 2, 1, 3)


_self_check()
