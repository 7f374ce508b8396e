/*
 * Native entry point of the per-prefix census of the route keys (integration/jni/bmq_jni.c, include/bmq.h: bmq_routes_prefix_census): what the
 * dist worker's split hinter asks its KV range per key prefix of a mutation batch, for all prefixes of the batch in one pass over the keys in
 * device memory.  NOT compiled in this repository (no JDK in its build image).
 *
 * A class of its own beside NativeGc, in its package: `engine` is the handle NativeMatcher.create returned; buffers are DIRECT buffers in
 * native byte order; a failure throws IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.routes.gpu;

import java.nio.ByteBuffer;
import java.nio.IntBuffer;
import java.nio.LongBuffer;

public final class NativeHinter {
    /** BMQ_PREFIX_MAX: the prefixes of one call at most */
    public static final int PREFIX_MAX = 65536;

    private NativeHinter() {
    }

    /** bmq_routes_prefix_census: prefix i is prefixes[prefixOff[i], prefixOff[i + 1]) (n + 1 offsets); outStats[4 i ..] = the live routes whose key
     *  starts with it with flag 1 (normal), 2 (unordered share), 3 (ordered share), and the sum of their key lengths.  Prefixes are compared as
     *  bytes, come in any order, may repeat and may nest (a key counts for every prefix that is a prefix of it); n <= PREFIX_MAX.  Read-only. */
    public static native void routesPrefixCensus(long engine, ByteBuffer prefixes, IntBuffer prefixOff, int n, LongBuffer outStats);
}
