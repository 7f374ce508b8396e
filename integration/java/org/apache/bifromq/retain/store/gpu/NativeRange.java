/*
 * Native entry points of the retain store's split and merge by KV boundary (integration/jni/bmq_jni.c, include/bmq.h): what
 * RetainStoreCoProc.reset(Boundary) needs instead of load(), the full KV scan (RetainStoreCoProc.java:133-137, 279-296).
 * NOT compiled in this repository (no JDK in its build image).
 *
 * `engine` is the handle NativeMatcher.create returned.  start / end: null = the side is absent, an empty array = present and empty (the
 * arguments of BoundaryUtil.inRange).  Failures other than a buffer that is too small throw IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.IntBuffer;

public final class NativeRange {
    private NativeRange() {
    }

    /** The retained topics whose retainMessageKey lies inside [start, end), decided where the index lives: out2 = {topics, key bytes (keys only)}. */
    public static native void retainCountIn(long engine, byte[] start, byte[] end, long[] out2);

    /** ... their ids, ascending. @return count, or -(needed) */
    public static native long retainIdsIn(long engine, byte[] start, byte[] end, IntBuffer outIds);

    /** retainCompactBegin for a range that SHRINKS: the next generation takes the topics inside the boundary only, and the swap replays
     *  only the logged adds / removes whose key lies inside; retainCompactBuild / retainCompactSwap / retainCompactAbort as before. */
    public static native void retainCompactBeginIn(long engine, byte[] start, byte[] end);

    /** RetainStoreCoProc.reset(Boundary) in ONE call: retainCompactBeginIn, the build (no engine lock held: matching and add / remove go on) and the
     *  swap; a failure behind the begin aborts the half-built generation.  out2 = {topics kept, logged ops replayed}. */
    public static native void retainReset(long engine, byte[] start, byte[] end, long[] out2);

    /** Every retained topic of src inside the boundary goes into dst with its stamps; an empty dst is bulk-loaded.  src serves on meanwhile.
     *  out2 = {imported, replaced (dst held the topic already: its stamps were replaced)}. */
    public static native void retainImport(long dst, long src, byte[] start, byte[] end, long[] out2);
}
