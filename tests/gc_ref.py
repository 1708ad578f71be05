"""A plain restatement of zbackup's garbage collection with Python sets: the
yardstick for zc_gc_plan.  It walks index file, bundle and record one after the
other, exactly as ChunkIndex::loadIndex drives BundleCollector
(chunk_index.cc:26-79, backup_collector.cc:17-144), with Writer::add's rules
for what is copied and where (chunk_storage.cc:31-46, chunk_index.cc:185-202).

    indexes[i] = [(bundle id, [(chunk id blob, size), ...]), ...]
    used       = iterable of chunk id blobs

plan() returns a dict of plain lists in the C ABI's terms (include/zchunk.h):
record numbers count the records in the order given (index, bundle, record).
A few hand-worked cases are checked on import, as aes_ref.py does."""

DEEP, REPACK, CONCAT = 1, 2, 4
KEEP, REMOVE, REPACK_BUNDLE, DROP_RECORD = 0, 1, 2, 3
COUNTED, USED, COPIED = 1, 2, 4
MAX_PAYLOAD_SIZE = 0x200000


class SizeMismatch(ValueError):
    """Two records with one id and different sizes: no defined result."""


def plan(indexes, used, flags=0, max_payload=MAX_PAYLOAD_SIZE):
    deep, repack, concat = bool(flags & DEEP), bool(flags & REPACK), bool(flags & CONCAT)
    used_set = set(bytes(u) for u in used)          # usedChunkSet
    overall_chunks, overall_bundles = set(), set()  # overallChunkSet, overallBundleSet
    reindex = set()                                 # the fresh ChunkIndex Writer::add fills
    size_of = {}
    record_flags, bundle_total, bundle_used, bundle_action, index_out = [], [], [], [], []
    copy, copy_bundle, copy_off, new_bundle_index, new_bundle_size = [], [], [], [], []
    first_rec = 0
    for i, bundles in enumerate(indexes):
        # startIndex
        x = dict(total=0, used=0, kept=0, modified_bundles=0, removed=0, modified=False, necessary=False)
        current = None  # the Writer's current bundle: its number among the new ones
        for bundle_id, records in bundles:
            bundle_id = bytes(bundle_id)
            k = len(records)
            flags_here = [0] * k
            total = n_used = 0
            # loadIndex: the records from the last to the first -> processChunk
            for r in range(k - 1, -1, -1):
                cid, size = bytes(records[r][0]), int(records[r][1])
                if size_of.setdefault(cid, size) != size:
                    raise SizeMismatch(cid.hex())
                if cid in used_set:
                    flags_here[r] |= USED
                if deep:
                    if cid in overall_chunks:
                        continue
                    overall_chunks.add(cid)
                flags_here[r] |= COUNTED
                total += 1
                if cid in used_set:
                    n_used += 1
                    x["necessary"] = True
            # finishBundle
            x["total"] += total
            x["used"] += n_used
            copies = False
            if n_used == 0 and total != 0:
                action = REMOVE
                x["modified"] = True
                x["removed"] += 1
            elif n_used < total or repack:
                action = REPACK_BUNDLE
                x["modified"] = True
                x["modified_bundles"] += 1
                copies = True
            elif deep and total == 0:
                x["modified"] = True
                if bundle_id not in overall_bundles:
                    overall_bundles.add(bundle_id)
                    action = REMOVE
                    x["removed"] += 1
                else:
                    action = DROP_RECORD
            else:
                if deep:
                    overall_bundles.add(bundle_id)
                action = KEEP
                x["kept"] += 1
            if copies:
                # copyUsedChunks: last to first again, every used record -> Writer::add
                for r in range(k - 1, -1, -1):
                    cid, size = bytes(records[r][0]), int(records[r][1])
                    if cid not in used_set or cid in reindex:
                        continue
                    reindex.add(cid)  # index.addChunk accepted it
                    if current is None:  # getCurrentBundle() makes one
                        current = len(new_bundle_size)
                        new_bundle_size.append(0)
                        new_bundle_index.append(i)
                    if new_bundle_size[current] + size > max_payload:  # finishCurrentBundle(), a new one
                        current = len(new_bundle_size)
                        new_bundle_size.append(0)
                        new_bundle_index.append(i)
                    copy.append(first_rec + r)
                    copy_bundle.append(current)
                    copy_off.append(new_bundle_size[current])
                    new_bundle_size[current] += size
                    flags_here[r] |= COPIED
            record_flags += flags_here
            bundle_total.append(total)
            bundle_used.append(n_used)
            bundle_action.append(action)
            first_rec += k
        # finishIndex: commit() or reset() finishes the current bundle either way
        # (an unmodified index file copied nothing, so there is none under concat)
        x["unlink"] = x["modified"] or (deep and not x["necessary"]) or concat
        index_out.append(x)
    return dict(record_flags=record_flags, bundle_total=bundle_total, bundle_used=bundle_used,
                bundle_action=bundle_action, indexes=index_out, copy=copy, copy_bundle=copy_bundle,
                copy_off=copy_off, new_bundle_index=new_bundle_index, new_bundle_size=new_bundle_size)


def files_to_unlink(p):
    """(bundle numbers, index numbers) the collection unlinks."""
    return ([b for b, a in enumerate(p["bundle_action"]) if a in (REMOVE, REPACK_BUNDLE)],
            [i for i, x in enumerate(p["indexes"]) if x["unlink"]])


def _cid(n):
    return bytes([n]) * 24


def _self_check():
    a, b, c, d = (_cid(n) for n in (1, 2, 3, 4))
    B1, B2, B3 = (_cid(n) for n in (101, 102, 103))
    # one index file: a bundle all used, one half used, one unused, one empty
    idx = [[(B1, [(a, 10), (b, 20)]), (B2, [(c, 30), (d, 40)]), (B3, [(d, 40)]), (B1, [])]]
    p = plan(idx, [a, b, c, c, _cid(9)])
    assert p["bundle_total"] == [2, 2, 1, 0] and p["bundle_used"] == [2, 1, 0, 0]
    assert p["bundle_action"] == [KEEP, REPACK_BUNDLE, REMOVE, KEEP]
    assert p["record_flags"] == [COUNTED | USED, COUNTED | USED, COUNTED | USED | COPIED, COUNTED, COUNTED]
    assert p["copy"] == [2] and p["copy_bundle"] == [0] and p["copy_off"] == [0]
    assert p["new_bundle_index"] == [0] and p["new_bundle_size"] == [30]
    x = p["indexes"][0]
    assert (x["total"], x["used"], x["kept"], x["modified_bundles"], x["removed"]) == (5, 3, 2, 1, 1)
    assert x["modified"] and x["necessary"] and x["unlink"]
    assert files_to_unlink(p) == ([1, 2], [0])
    # repack: every bundle with a used chunk is rewritten, last record first; 35 bytes close a bundle
    p = plan(idx, [a, b, c], REPACK, max_payload=35)
    assert p["bundle_action"] == [REPACK_BUNDLE, REPACK_BUNDLE, REMOVE, REPACK_BUNDLE]
    assert p["copy"] == [1, 0, 2] and p["copy_bundle"] == [0, 0, 1] and p["copy_off"] == [0, 20, 0]
    assert p["new_bundle_size"] == [30, 30]
    # a chunk over max_payload finishes the empty bundle Writer::add has just made
    p = plan(idx, [c], 0, max_payload=29)
    assert p["copy"] == [2] and p["copy_bundle"] == [1] and p["new_bundle_size"] == [0, 30]
    # deep: the second index file repeats the first; its records are not counted, its bundle goes,
    # a third copy of the bundle only drops its record; an unused index file is unlinked
    idx2 = [[(B1, [(a, 10), (b, 20)])], [(B1, [(b, 20), (a, 10)])], [(B1, [(a, 10)])], [(B2, [(c, 30)])]]
    p = plan(idx2, [a, b], DEEP)
    assert p["record_flags"] == [COUNTED | USED, COUNTED | USED, USED, USED, USED, COUNTED]
    assert p["bundle_action"] == [KEEP, DROP_RECORD, DROP_RECORD, REMOVE]
    assert [x["unlink"] for x in p["indexes"]] == [False, True, True, True]
    assert [x["necessary"] for x in p["indexes"]] == [True, False, False, False]
    p = plan([[(B2, [(a, 10)])]] + idx2[1:], [a, b], DEEP)
    # b is first seen in index 1 now; a is not: bundle B1 there has total 1, used 1 -> kept; then
    # index 2's B1 (total 0) was seen -> DROP_RECORD
    assert p["bundle_action"] == [KEEP, KEEP, DROP_RECORD, REMOVE]
    # deep, total 0, id never seen: the bundle file is removed
    p = plan([[(B1, [(a, 10)])], [(B3, [(a, 10)]), (B3, [(a, 10)])]], [a], DEEP)
    assert p["bundle_action"] == [KEEP, REMOVE, DROP_RECORD]
    # without deep every record counts, wherever else its id is; the copy list still holds an id once,
    # and a new bundle never spans two index files
    p = plan([[(B1, [(a, 10), (c, 30)])], [(B2, [(d, 40), (a, 10)])]], [a])
    assert p["bundle_action"] == [REPACK_BUNDLE, REPACK_BUNDLE] and p["copy"] == [0]
    assert p["record_flags"] == [COUNTED | USED | COPIED, COUNTED, COUNTED, COUNTED | USED]
    p = plan([[(B1, [(a, 10), (c, 30)])], [(B2, [(d, 40), (b, 20)])]], [a, b])
    assert p["copy"] == [0, 3] and p["copy_bundle"] == [0, 1] and p["new_bundle_index"] == [0, 1]
    # concat unlinks every index file; nothing else changes
    p = plan(idx2[:1], [a, b], CONCAT)
    assert p["bundle_action"] == [KEEP] and p["indexes"][0]["unlink"] and not p["indexes"][0]["modified"]
    try:
        plan([[(B1, [(a, 10)]), (B2, [(a, 11)])]], [])
    except SizeMismatch:
        pass
    else:
        raise AssertionError("a size mismatch went unnoticed")
    assert plan([], []) == dict(record_flags=[], bundle_total=[], bundle_used=[], bundle_action=[], indexes=[],
                                copy=[], copy_bundle=[], copy_off=[], new_bundle_index=[], new_bundle_size=[])


_self_check()
