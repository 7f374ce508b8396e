/*
 * Native entry points of the reads in key order: a window of the route keys and the dist worker's GC sweep over it (integration/jni/bmq_jni.c,
 * include/bmq.h: bmq_routes_window, bmq_routes_gc_sweep).  NOT compiled in this repository (no JDK in its build image).
 *
 * A class of its own beside NativeRoutes, in its package (public: NativeMatcher and its adapters are package-private to the dist worker's): `engine` is the handle NativeMatcher.create returned; buffers are
 * DIRECT buffers in native byte order; a failure throws IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.routes.gpu;

import java.nio.ByteBuffer;
import java.nio.IntBuffer;
import java.nio.LongBuffer;

public final class NativeGc {
    private NativeGc() {
    }

    /** bmq_routes_window: the ids of the first maxRoutes (<= 65 536) live routes whose key is >= lo[0, loLen) (> with exclusive; lo null: from the
     *  first key) -> outIds in KV order, the count returned; outMore[0] = 1 if a further live key follows.  What an IKVIterator gives after seek(lo):
     *  ordered on the device, the keys stay there.  FanoutSplitHinter.doEstimate is one call: seek(prefix), splitAtScale steps. */
    public static native int routesWindow(long engine, ByteBuffer lo, int loLen, boolean exclusive, int maxRoutes, IntBuffer outIds, IntBuffer outMore);

    /** bmq_routes_gc_sweep: the loop of DistWorkerCoProc.gc (DistWorkerCoProc.java:554-701) over the key order -> the inspected route ids in
     *  inspection order in outIds, their count returned; -(needed) if cap is too small (nothing else is valid then).  startKey null: absent.
     *  reply[0] = wrapped, reply[1] = hasNextStartKey, reply[2] = the route id of nextStartKey (routeKey below gives its bytes),
     *  reply[3] = the engine epoch the sweep saw. */
    public static native int routesGcSweep(long engine, ByteBuffer startKey, int startLen, int stepHint, int scanQuota, IntBuffer outIds, int cap, LongBuffer reply);

    /** bmq_route_key: the key bytes of a live route -> out, the length returned; -(the length needed) if out is too small.  The same call as
     *  NativeMatcher.routeKey, reachable from this package: how nextStartKey becomes bytes. */
    public static native int routeKey(long engine, int routeId, ByteBuffer out);
}
