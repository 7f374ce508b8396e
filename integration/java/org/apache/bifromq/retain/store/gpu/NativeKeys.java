/*
 * Native entry points that compose retainMessageKey(tenant, topic) on the device (integration/jni/bmq_jni.c, include/bmq.h:
 * bmq_retain_keys_by_id, bmq_retain_keys_prepare, bmq_retain_keys_match).  NOT compiled in this repository (no JDK in its build image).
 *
 * A class of its own beside NativeStore, whose set of natives is what GpuRetainGc / GpuTenantsStats use and nothing else.  `engine` is the
 * handle NativeMatcher.create returned; buffers are DIRECT buffers in native byte order; failures other than a buffer that is too small throw
 * IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.IntBuffer;
import java.nio.LongBuffer;

public final class NativeKeys {
    private NativeKeys() {
    }

    /** NativeStore.retainMessageKeys composed ON THE DEVICE: two kernels on the engine stream over the generation's device-resident string store, no
     *  host copy of the dead bitmap.  The same contract and the same bytes: outOff[n + 1] byte offsets into out; an id that is unknown or not
     *  retained now gives an empty key. @return bytes, or -(needed) */
    public static native long retainKeysById(long engine, IntBuffer ids, int n, ByteBuffer out, LongBuffer outOff);

    /** Builds the string store of the current generation now (otherwise the first retainKeysById / retainMatchKeys after a bulk load does).
     *  @return the bytes it holds on the device */
    public static native long retainKeysPrepare(long engine);

    /** NativeMatcher.retainMatchLimited (the same arguments, rows, ids and counts) plus retainMessageKey(tenant, topic) of every kept id in row order
     *  (outKeyOff[kept + 1] byte offsets into outKeys): the keys RetainStoreCoProc.match hands to reader.get, composed on the device where the kept
     *  ids lie.  needed2 = {kept ids, key bytes}, always. @return kept ids, or -1 when a buffer was too small */
    public static native long retainMatchKeys(long engine, ByteBuffer tenants, IntBuffer tenantOff, int nTenants,
                                              IntBuffer filterTenant, ByteBuffer filters, IntBuffer filterOff, int nFilters,
                                              IntBuffer limits, long nowMs, IntBuffer outRowPtr, IntBuffer outTopicIds,
                                              IntBuffer outCounts, LongBuffer outKeyOff, ByteBuffer outKeys, long[] needed2);
}
