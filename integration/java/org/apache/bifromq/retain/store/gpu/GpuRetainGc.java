/*
 * RetainStoreCoProc.gc (bifromq-retain/bifromq-retain-store/src/main/java/org/apache/bifromq/retain/store/RetainStoreCoProc.java:257-277) over the
 * engine's topic ids, beside the IRetainTopicIndex drop-in (GpuRetainTopicIndex): the scan, the KV keys to delete and the post-commit removal
 * from the index are one native call each, and the removal goes BY ID -- the ids name their slots, nothing is encoded, uploaded again as
 * strings or looked up level by level.
 * NOT compiled in this repository (no JDK in its build image).
 *
 *   Expired e = gc.expired(tenantId, now, expirySeconds);
 *   for k in 0 .. e.n: writer.delete(e.keys[e.keyOff[k], e.keyOff[k + 1]));  // an empty key: removed since the scan
 *   ... commit ...
 *   gc.removeExpired(e);                                                // the post-commit closure (:270-275)
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.IntBuffer;
import java.nio.LongBuffer;
import java.nio.charset.StandardCharsets;

public final class GpuRetainGc {
    private final long engine;

    public GpuRetainGc(long engine) {
        this.engine = engine;
    }

    private static ByteBuffer direct(int bytes) {
        return ByteBuffer.allocateDirect(bytes).order(ByteOrder.nativeOrder());
    }

    /** The expired topics of RetainStoreCoProc.gc (RetainStoreCoProc.java:257-277) as the engine's ids plus the KV keys to delete, one native call
     *  each: the scan runs on the device, the keys come back as bytes.  Hand the result to removeExpired AFTER the KV commit. */
    public static final class Expired {
        public final IntBuffer ids;
        public final int n;
        public final long generation;
        public final ByteBuffer keys;
        public final LongBuffer keyOff; // key k = keys[keyOff[k], keyOff[k + 1]); empty: removed since the scan

        Expired(IntBuffer ids, int n, long generation, ByteBuffer keys, LongBuffer keyOff) {
            this.ids = ids;
            this.n = n;
            this.generation = generation;
            this.keys = keys;
            this.keyOff = keyOff;
        }
    }

    public Expired expired(String tenantId, long nowMs, long overrideExpirySeconds) {
        long generation = NativeStore.retainGeneration(engine); // before the scan: a bulk load in between makes removeExpired throw
        byte[] tn = tenantId == null ? null : tenantId.getBytes(StandardCharsets.UTF_8);
        IntBuffer ids = direct(4 * 4096).asIntBuffer();
        long got = NativeStore.retainExpired(engine, tn, nowMs, overrideExpirySeconds, ids);
        while (got < 0) {
            ids = direct((int) (4 * -got)).asIntBuffer();
            got = NativeStore.retainExpired(engine, tn, nowMs, overrideExpirySeconds, ids);
        }
        int n = (int) got;
        LongBuffer off = direct(8 * (n + 1)).asLongBuffer();
        ByteBuffer keys = direct(Math.max(4096, 96 * n));
        long bytes = NativeStore.retainMessageKeys(engine, ids, n, keys, off);
        while (bytes < 0) {
            keys = direct((int) -bytes);
            bytes = NativeStore.retainMessageKeys(engine, ids, n, keys, off);
        }
        return new Expired(ids, n, generation, keys, off);
    }

    /** The post-commit closure of gc (RetainStoreCoProc.java:270-275): the ids name their slots, nothing is encoded, uploaded or looked up level
     *  by level.  A bulk load in between (another generation of ids) makes the call throw: scan again. */
    public long removeExpired(Expired e) {
        return e.n == 0 ? 0 : NativeStore.retainRemoveIds(engine, e.ids, e.n, e.generation);
    }
}
