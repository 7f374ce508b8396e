/*
 * The per-tenant numbers both co-processors keep beside their indexes, read from the engine instead of a KV scan.
 * NOT compiled in this repository (no JDK in its build image).
 *
 * Dist worker: TenantsStats.doReset (bifromq-dist/bifromq-dist-worker/src/main/java/org/apache/bifromq/dist/worker/TenantsStats.java:229-246)
 * walks every key of the range on every IKVRangeCoProc.reset and counts normal and shared routes per tenant from the key's flag; the
 * space gauge asks reader.size(tenantSection) per tenant (:140-162).  routes() is one native call for all tenants: the engine passes
 * once over the key references it holds in device memory (bmq_routes_tenant_stats).  A tenant without routes inside the boundary
 * is absent, as TenantsStats destroys an entry at isNoRoutes; a shared-subscription key counts once, as doAddSharedRoutes(tenantId, 1).
 * Retain store: RetainStoreCoProc.load() (bifromq-retain/bifromq-retain-store/.../RetainStoreCoProc.java:279-296) counts topics per tenant
 * while it scans; retainedTopics() is the same count from the index (bmq_retain_tenant_counts).
 * Public, in a package of its own: the dist worker's co-processor (org.apache.bifromq.dist.worker.gpu) and the retain store's both use it.
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.LongBuffer;
import java.nio.charset.StandardCharsets;
import java.util.LinkedHashMap;
import java.util.Map;

public final class GpuTenantsStats {
    /** What TenantsStats keeps per tenant. */
    public static final class Routes {
        public final long normal;
        public final long unorderedShare;
        public final long orderedShare;
        public final long keyBytes; // keys only

        Routes(long normal, long unorderedShare, long orderedShare, long keyBytes) {
            this.normal = normal;
            this.unorderedShare = unorderedShare;
            this.orderedShare = orderedShare;
            this.keyBytes = keyBytes;
        }

        public long sharedRoutes() {
            return unorderedShare + orderedShare;
        }

        /** reader.size(tenantSection): a normal route's value is 8 bytes (the incarnation); a group's value lives in the KV store. */
        public long spaceLowerBound() {
            return keyBytes + 8 * normal;
        }
    }

    private final long engine;

    /** engine: the handle NativeMatcher.create returned (both co-processors of a store share it). */
    public GpuTenantsStats(long engine) {
        this.engine = engine;
    }

    private static ByteBuffer direct(int bytes) {
        return ByteBuffer.allocateDirect(bytes).order(ByteOrder.nativeOrder());
    }

    private static String name(ByteBuffer names, LongBuffer off, int i) {
        byte[] raw = new byte[(int) (off.get(i + 1) - off.get(i))];
        ByteBuffer at = names.duplicate(); // (an absolute bulk get exists from Java 13 on only)
        at.position((int) off.get(i));
        at.get(raw);
        return new String(raw, StandardCharsets.UTF_8);
    }

    /** Tenants with a live route inside [start, end) (null: the side is absent), in byte order of their ids. */
    public Map<String, Routes> routes(byte[] start, byte[] end) {
        int cap = 256, nameBytes = 8192;
        long[] needed = new long[2];
        for (;;) {
            ByteBuffer names = direct(nameBytes);
            LongBuffer off = direct(8 * (cap + 1)).asLongBuffer(), stats = direct(32 * cap).asLongBuffer();
            long n = NativeStore.routesTenantStats(engine, start, end, names, off, stats, needed);
            if (n < 0) {
                cap = (int) Math.max(cap, needed[0]);
                nameBytes = (int) Math.max(nameBytes, needed[1]);
                continue;
            }
            Map<String, Routes> out = new LinkedHashMap<>();
            for (int i = 0; i < n; i++) {
                out.put(name(names, off, i), new Routes(stats.get(4 * i), stats.get(4 * i + 1), stats.get(4 * i + 2), stats.get(4 * i + 3)));
            }
            return out;
        }
    }

    /** Retained topics per tenant now ('$' topics included), in byte order of the tenant ids. */
    public Map<String, Long> retainedTopics() {
        int cap = 256, nameBytes = 8192;
        long[] needed = new long[2];
        for (;;) {
            ByteBuffer names = direct(nameBytes);
            LongBuffer off = direct(8 * (cap + 1)).asLongBuffer(), counts = direct(8 * cap).asLongBuffer();
            long n = NativeStore.retainTenantCounts(engine, names, off, counts, needed);
            if (n < 0) {
                cap = (int) Math.max(cap, needed[0]);
                nameBytes = (int) Math.max(nameBytes, needed[1]);
                continue;
            }
            Map<String, Long> out = new LinkedHashMap<>();
            for (int i = 0; i < n; i++) {
                out.put(name(names, off, i), counts.get(i));
            }
            return out;
        }
    }
}
