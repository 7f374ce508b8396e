/*
 * Native entry points of the two halves of RetainStoreCoProc.batchRetain around the KV commit (integration/jni/bmq_jni.c, include/bmq.h:
 * bmq_retain_plan, bmq_retain_plan_commit).  NOT compiled in this repository (no JDK in its build image).
 *
 * A class of its own beside NativeStore / NativeKeys.  `engine` is the handle NativeMatcher.create returned; buffers are DIRECT buffers in
 * native byte order; failures other than a key buffer that is too small throw IllegalStateException with bmq_last_error().
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.IntBuffer;
import java.nio.LongBuffer;

public final class NativeRetainPlan {
    /** out_action of retainPlan (BMQ_PLAN_* of include/bmq.h) */
    public static final int NONE = 0, ADD = 1, UPDATE = 2, REMOVE = 3, SUPERSEDED = 4;
    /** out_code of retainPlan: RetainResult.Code numbers (RetainStoreCoProc.proto) */
    public static final int RETAINED = 0, CLEARED = 1;

    private NativeRetainPlan() {
    }

    /** The pre-commit half, read-only, for n ops (opTenant[i] indexes the tenant table, null: tenant 0; topicOff[n + 1]; clear[i] != 0: the payload is
     *  empty).  Ops with equal tenant bytes and topic bytes form a group whose LAST op wins.  Per op: outCode (the winner's), outAction, outWinner,
     *  outTopicId (0xFFFFFFFF: not retained now); per tenant-table entry: outDelta (the topic-count change); the winners' retainMessageKeys at
     *  outKeyOff[n + 1] into outKeys (empty for NONE and SUPERSEDED).  info8 = {generation, epoch, groups, add, update, remove, none, key bytes}.
     *  @return key bytes, or -(needed) when outKeys was too small (everything but the key bytes has been written) */
    public static native long retainPlan(long engine, ByteBuffer tenants, IntBuffer tenantOff, int nTenants, IntBuffer opTenant, ByteBuffer topics,
                                         IntBuffer topicOff, ByteBuffer clear, int n, ByteBuffer outCode, ByteBuffer outAction, IntBuffer outWinner,
                                         IntBuffer outTopicId, IntBuffer outDelta, LongBuffer outKeyOff, ByteBuffer outKeys, long[] info8);

    /** The post-commit closure for the same op arrays and the plan's outAction: winners with ADD / UPDATE are added (timestampHlc / expirySeconds per op,
     *  both null: none), winners with REMOVE are removed.  Throws IllegalStateException -- nothing is applied -- when (generation, epoch) of info8 are
     *  not the index's any more.  outTopicIds (may be null): the id of every winner that changed the index, else 0xFFFFFFFF. */
    public static native void retainPlanCommit(long engine, ByteBuffer tenants, IntBuffer tenantOff, int nTenants, IntBuffer opTenant, ByteBuffer topics,
                                               IntBuffer topicOff, int n, ByteBuffer action, LongBuffer timestampHlc, IntBuffer expirySeconds,
                                               long generation, long epoch, IntBuffer outTopicIds);
}
