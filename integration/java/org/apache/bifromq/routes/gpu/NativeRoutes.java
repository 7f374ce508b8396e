/*
 * Native entry point that turns route keys into route ids where the route index lives (integration/jni/bmq_jni.c, include/bmq.h:
 * bmq_routes_find).  NOT compiled in this repository (no JDK in its build image).
 *
 * A class of its own beside NativeMatcher, like NativeKeys / NativeStore / NativeRange: `engine` is the handle NativeMatcher.create
 * returned; buffers are DIRECT buffers in native byte order; a failure throws IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.routes.gpu;

import java.nio.ByteBuffer;
import java.nio.IntBuffer;

public final class NativeRoutes {
    private NativeRoutes() {
    }

    /** bmq_routes_find: outIds[i] = id of the live route whose key is keys[keyOff[i] .. keyOff[i + 1]), 0xFFFFFFFF (-1) if there is none; keys in
     *  the layout NativeMatcher.rebuild / routesApply take, any order, repeats included; read-only (one lane per key walks the index on the device).
     *  After the post-commit NativeMatcher.routesApply the adapter asks for the ids of the keys it put: a put of a key that was already there keeps
     *  its old id, so the ids cannot be inferred from indexInfo's nextRouteId.  A malformed key throws, as it does in routesApply. */
    public static native void routesFind(long engine, ByteBuffer keys, IntBuffer keyOff, int n, IntBuffer outIds);
}
