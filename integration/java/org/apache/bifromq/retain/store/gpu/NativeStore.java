/*
 * Native entry points of the per-tenant statistics and of the retain GC by id (integration/jni/bmq_jni.c, include/bmq.h).
 * NOT compiled in this repository (no JDK in its build image).
 *
 * `engine` is the handle NativeMatcher.create returned: both co-processors of a store share it.  Buffers are DIRECT buffers in native byte
 * order, as for NativeMatcher; failures other than a buffer that is too small throw IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.IntBuffer;
import java.nio.LongBuffer;

public final class NativeStore {
    private NativeStore() {
    }

    /** The scan of RetainStoreCoProc.gc on the device: ids (ascending) whose message has expired at nowMs -- of every tenant (tenant == null) or of
     *  one (its '$' topics are out of reach, as for the reference's match(tenantId, "#")); overrideExpirySeconds < 0: none. @return count, or -(needed) */
    public static native long retainExpired(long engine, byte[] tenant, long nowMs, long overrideExpirySeconds, IntBuffer outIds);

    /** The generation the engine's topic ids belong to now (+1 per bulk load): read it BEFORE the scan whose ids go to retainRemoveIds. */
    public static native long retainGeneration(long engine);

    /** retainMessageKey(tenant, topic) of every id: the keys gc deletes and match gets.  outOff[n + 1] byte offsets into out; an id that is unknown or
     *  not retained now gives an empty key. @return bytes, or -(needed) */
    public static native long retainMessageKeys(long engine, IntBuffer ids, int n, ByteBuffer out, LongBuffer outOff);

    /** The post-commit half of gc BY ID (ids of retainExpired / retainLiveIds / a match, of `generation` = retainGeneration read before): dead ids and
     *  repeats are no-ops. @return topics removed.  Throws if the generation has changed or an id was never handed out (nothing is changed then). */
    public static native long retainRemoveIds(long engine, IntBuffer ids, int n, long generation);

    /** Retained topics per tenant ('$' topics included), in byte order of the tenant ids: what RetainStoreCoProc.load() counts while it scans.
     *  outTenantOff[n + 1] byte offsets into outTenants. @return tenants, or -1 with needed2 = {tenants, id bytes} when a buffer was too small */
    public static native long retainTenantCounts(long engine, ByteBuffer outTenants, LongBuffer outTenantOff, LongBuffer outCounts, long[] needed2);

    /** The census TenantsStats.doReset takes by walking the range, from the keys the engine holds: per tenant with a live route inside [start, end)
     *  (null: the side is absent), in byte order of the ids, outStats[4 i ..] = {normal routes, unordered shares, ordered shares, key bytes}; a shared
     *  subscription key counts once; key bytes are keys only (reader.size adds the 8-byte value of every normal route).
     *  @return tenants, or -1 with needed2 = {tenants, id bytes} when a buffer was too small */
    public static native long routesTenantStats(long engine, byte[] start, byte[] end, ByteBuffer outTenants, LongBuffer outTenantOff, LongBuffer outStats,
                                                long[] needed2);
}
