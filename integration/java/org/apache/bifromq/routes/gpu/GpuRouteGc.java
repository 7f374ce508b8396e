/*
 * DistWorkerCoProc.gc (bifromq-dist/bifromq-dist-worker/src/main/java/org/apache/bifromq/dist/worker/DistWorkerCoProc.java:554-701) without the
 * RocksDB iterator: the engine walks its own route keys in key order on the device (NativeGc.routesGcSweep) and answers with the inspected route
 * ids, wrapped and nextStartKey; what follows per inspected route stays here, as in the reference -- the routeCache.isCached filter, the members
 * of a group route, the CheckRequest per (subBrokerId, delivererKey, tenant) and removeSuccess from the checker's answers.
 * NOT compiled in this repository (no JDK in its build image).
 *
 *   Sweep s = gc.sweep(request, boundary);
 *   for k in 0 .. s.n: Matching m = routes.matching(s.ids.get(k));     // the adapter's id -> (key, value) table, as GpuTenantRouteMatcher keeps it
 *                      if (!routeCache.isCached(m.tenantId(), m.matcher.getFilterLevelList())) add m (or its receiverList) to the CheckRequests
 *   reply.setInspectedCount(s.n).setWrapped(s.wrapped); if (s.nextStartKey != null) reply.setNextStartKey(s.nextStartKey);
 */
package org.apache.bifromq.routes.gpu;

import com.google.protobuf.ByteString;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.IntBuffer;
import java.nio.LongBuffer;
import org.apache.bifromq.basekv.proto.Boundary;
import org.apache.bifromq.basekv.utils.BoundaryUtil;
import org.apache.bifromq.dist.rpc.proto.GCRequest;

public final class GpuRouteGc {
    private final long engine;

    public GpuRouteGc(long engine) {
        this.engine = engine;
    }

    public static final class Sweep {
        public final IntBuffer ids; // the inspected routes, in inspection order
        public final int n;
        public final boolean wrapped;
        public final ByteString nextStartKey; // null: none
        public final long epoch;

        Sweep(IntBuffer ids, int n, boolean wrapped, ByteString nextStartKey, long epoch) {
            this.ids = ids;
            this.n = n;
            this.wrapped = wrapped;
            this.nextStartKey = nextStartKey;
            this.epoch = epoch;
        }
    }

    private static ByteBuffer direct(int bytes) {
        return ByteBuffer.allocateDirect(bytes).order(ByteOrder.nativeOrder());
    }

    public Sweep sweep(GCRequest request, Boundary boundary) {
        int step = Math.max(request.getStepHint(), 1);
        int quota = request.getScanQuota() > 0 ? request.getScanQuota() : 256 * step;
        ByteString startKey = null;
        if (request.hasStartKey()) { // the clamp of :563-574: the engine holds exactly its range's keys and takes no boundary
            startKey = request.getStartKey();
            if (boundary != null) {
                ByteString startBoundary = BoundaryUtil.startKey(boundary);
                if (BoundaryUtil.compareStartKey(startKey, startBoundary) < 0
                    || BoundaryUtil.compareEndKeys(startKey, BoundaryUtil.endKey(boundary)) >= 0) {
                    startKey = startBoundary;
                }
            }
        }
        ByteBuffer lo = null;
        if (startKey != null) {
            lo = direct(Math.max(startKey.size(), 1));
            startKey.copyTo(lo);
        }
        IntBuffer ids = direct(4 * quota).asIntBuffer();
        LongBuffer reply = direct(8 * 4).asLongBuffer();
        int n = NativeGc.routesGcSweep(engine, lo, startKey == null ? 0 : startKey.size(), request.getStepHint(), request.getScanQuota(), ids, quota, reply);
        if (n < 0) {
            throw new IllegalStateException("a sweep inspects at most its quota");
        }
        ByteString next = null;
        if (reply.get(1) != 0) {
            ByteBuffer key = direct(512);
            int len = NativeGc.routeKey(engine, (int) reply.get(2), key);
            if (len < 0) { // -(the length needed)
                key = direct(-len);
                len = NativeGc.routeKey(engine, (int) reply.get(2), key);
            }
            key.limit(len);
            next = ByteString.copyFrom(key);
        }
        return new Sweep(ids, n, reply.get(0) != 0, next, reply.get(3));
    }
}
