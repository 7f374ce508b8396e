/*
 * RetainStoreCoProc.reset(Boundary) (bifromq-retain/bifromq-retain-store/src/main/java/org/apache/bifromq/retain/store/RetainStoreCoProc.java:133-137)
 * WITHOUT load(), the scan of the whole range (:279-296), beside the IRetainTopicIndex drop-in (GpuRetainTopicIndex) over the same engine handle:
 * the index holds no KV keys, so the engine evaluates start <= retainMessageKey(id) < end over its own topic ids.
 * NOT compiled in this repository (no JDK in its build image).
 *
 *   split of range A at key s:   b.importFrom(a, s, null);  a.reset(null, s);      // the sibling first, then the range that shrinks
 *   merge of B into A:           a.importFrom(b, null, null);
 *
 * start / end: null = the side is absent, an empty array = present and empty (the arguments of BoundaryUtil.inRange).  Topic ids are re-numbered
 * by reset and by an import into an empty engine (NativeStore.retainGeneration): ids held across either are refused by retainRemoveIds.
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.IntBuffer;

public final class GpuRetainRange {
    private final long engine;

    public GpuRetainRange(long engine) {
        this.engine = engine;
    }

    /** After a split the range keeps the keys of [start, end): the next generation is built from the topics inside, beside the serving one, which
     *  goes on matching and mutating over ALL its topics until the swap; mutations logged meanwhile are replayed only if their key lies inside.
     *  The tenant counts behind the coproc's gauges follow with NativeStore.retainTenantCounts.  @return {topics kept, ops replayed} */
    public long[] reset(byte[] start, byte[] end) {
        long[] out = new long[2];
        if (start == null && end == null) { // FULL_BOUNDARY: the range owns what it holds
            NativeRange.retainCountIn(engine, null, null, out);
            out[1] = 0;
            return out;
        }
        NativeRange.retainReset(engine, start, end, out);
        return out;
    }

    /** {retained topics whose key lies inside [start, end), their key bytes}: reader.size(boundary) of the keys, from the index. */
    public long[] count(byte[] start, byte[] end) {
        long[] out = new long[2];
        NativeRange.retainCountIn(engine, start, end, out);
        return out;
    }

    /** The engine's ids of the retained topics inside [start, end), ascending (for NativeStore.retainMessageKeys / NativeKeys.retainKeysById). */
    public IntBuffer idsIn(byte[] start, byte[] end) {
        IntBuffer ids = ByteBuffer.allocateDirect(4 * 4096).order(ByteOrder.nativeOrder()).asIntBuffer();
        long got = NativeRange.retainIdsIn(engine, start, end, ids);
        while (got < 0) {
            ids = ByteBuffer.allocateDirect((int) (4 * -got)).order(ByteOrder.nativeOrder()).asIntBuffer();
            got = NativeRange.retainIdsIn(engine, start, end, ids);
        }
        ids.limit((int) got);
        return ids;
    }

    /** Every retained topic of `src` inside [start, end) comes into this range's index with its stamps, without a KV scan; `src` serves on
     *  meanwhile.  An empty index is bulk-loaded.  @return {imported, replaced} */
    public long[] importFrom(GpuRetainRange src, byte[] start, byte[] end) {
        long[] out = new long[2];
        NativeRange.retainImport(engine, src.engine, start, end, out);
        return out;
    }
}
