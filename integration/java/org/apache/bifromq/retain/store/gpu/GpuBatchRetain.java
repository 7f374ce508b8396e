/*
 * RetainStoreCoProc.batchRetain (bifromq-retain/bifromq-retain-store/src/main/java/org/apache/bifromq/retain/store/RetainStoreCoProc.java:193-255)
 * on top of NativeRetainPlan: the index lookups, the CLEARED / RETAINED decision, the KV keys and the add / update / remove filing of a whole
 * batch are ONE native call in front of the KV commit, the index mutation one behind it.
 * NOT compiled in this repository (no JDK in its build image).
 *
 *   Plan p = batch.plan(tenantIds, opTenant, topics, payloadEmpty);
 *   for i in 0 .. p.n:
 *       if (p.action(i) == ADD || p.action(i) == UPDATE) writer.put(p.key(i), topicMessage(i).toByteString());   // :225 / :230
 *       if (p.action(i) == REMOVE) writer.delete(p.key(i));                                                      // :217
 *       results.put(topic(i), p.code(i) == CLEARED ? Code.CLEARED : Code.RETAINED);                              // :220 / :234, the winner's for every op
 *   return () -> {                                                                                               // :240-255
 *       batch.commit(p, timestamps, expiryIntervals);
 *       for t in 0 .. tenantIds.length: tenantsStats.increaseTopicCount(tenantIds[t], p.delta(t));
 *   };
 * Requests of one topic keep BatchRetainCallHelper.makeBatch's rule: the last one wins, the others are SUPERSEDED and write nothing.
 */
package org.apache.bifromq.retain.store.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.IntBuffer;
import java.nio.LongBuffer;
import java.nio.charset.StandardCharsets;

public final class GpuBatchRetain {
    private final long engine;

    public GpuBatchRetain(long engine) {
        this.engine = engine;
    }

    private static ByteBuffer direct(int bytes) {
        return ByteBuffer.allocateDirect(Math.max(bytes, 16)).order(ByteOrder.nativeOrder());
    }

    /** A batch's ops as the natives take them, and what retainPlan said about them.  Hand it to commit AFTER the KV commit. */
    public static final class Plan {
        public final int n;
        final int nTenants;
        final ByteBuffer tenants, topics, clear, code, action;
        final IntBuffer tenantOff, opTenant, topicOff, winner, topicId, delta;
        final LongBuffer keyOff;
        ByteBuffer keys;
        final long[] info = new long[8]; // generation, epoch, groups, add, update, remove, none, key bytes

        Plan(int n, int nTenants, int tenantBytes, int topicBytes) {
            this.n = n;
            this.nTenants = nTenants;
            tenants = direct(tenantBytes + 16);
            topics = direct(topicBytes + 16);
            clear = direct(n);
            code = direct(n);
            action = direct(n);
            tenantOff = direct(4 * (nTenants + 1)).asIntBuffer();
            opTenant = direct(4 * n).asIntBuffer();
            topicOff = direct(4 * (n + 1)).asIntBuffer();
            winner = direct(4 * n).asIntBuffer();
            topicId = direct(4 * n).asIntBuffer();
            delta = direct(4 * nTenants).asIntBuffer();
            keyOff = direct(8 * (n + 1)).asLongBuffer();
            keys = direct(Math.max(4096, 96 * n));
        }

        public int action(int i) {
            return action.get(i);
        }

        public int code(int i) {
            return code.get(i);
        }

        public int winner(int i) {
            return winner.get(i);
        }

        /** the topic's id in the index if it is retained now, -1 (0xFFFFFFFF) otherwise */
        public int topicId(int i) {
            return topicId.get(i);
        }

        /** the change of tenant t's retained-topic count this batch makes */
        public int delta(int t) {
            return delta.get(t);
        }

        /** retainMessageKey(tenant, topic) of op i: the key of its put or delete; empty for NONE and SUPERSEDED */
        public byte[] key(int i) {
            byte[] k = new byte[(int) (keyOff.get(i + 1) - keyOff.get(i))];
            ByteBuffer v = keys.duplicate();
            v.position((int) keyOff.get(i));
            v.get(k);
            return k;
        }
    }

    public Plan plan(String[] tenantIds, int[] opTenant, String[] topics, boolean[] payloadEmpty) {
        byte[][] tn = new byte[tenantIds.length][], tp = new byte[topics.length][];
        int tb = 0, pb = 0;
        for (int t = 0; t < tn.length; t++) {
            tn[t] = tenantIds[t].getBytes(StandardCharsets.UTF_8);
            tb += tn[t].length;
        }
        for (int i = 0; i < tp.length; i++) {
            tp[i] = topics[i].getBytes(StandardCharsets.UTF_8);
            pb += tp[i].length;
        }
        Plan p = new Plan(topics.length, tn.length, tb, pb);
        p.tenantOff.put(0, 0);
        for (int t = 0, at = 0; t < tn.length; t++) {
            p.tenants.put(tn[t]);
            p.tenantOff.put(t + 1, at += tn[t].length);
        }
        p.topicOff.put(0, 0);
        for (int i = 0, at = 0; i < tp.length; i++) {
            p.topics.put(tp[i]);
            p.topicOff.put(i + 1, at += tp[i].length);
            p.opTenant.put(i, opTenant[i]);
            p.clear.put(i, (byte) (payloadEmpty[i] ? 1 : 0));
        }
        long bytes = NativeRetainPlan.retainPlan(engine, p.tenants, p.tenantOff, p.nTenants, p.opTenant, p.topics, p.topicOff, p.clear, p.n, p.code, p.action,
            p.winner, p.topicId, p.delta, p.keyOff, p.keys, p.info);
        if (bytes < 0) { // the key buffer was too small: everything else is there, the second call fetches the bytes
            p.keys = direct((int) -bytes);
            NativeRetainPlan.retainPlan(engine, p.tenants, p.tenantOff, p.nTenants, p.opTenant, p.topics, p.topicOff, p.clear, p.n, p.code, p.action,
                p.winner, p.topicId, p.delta, p.keyOff, p.keys, p.info);
        }
        return p;
    }

    /** The post-commit closure (RetainStoreCoProc.java:240-255).  Throws IllegalStateException if the index has changed since plan(): the caller
     *  serialises mutations of a range (the reference runs batchRetain under the range's single writer), so that is a bug, not a race to retry. */
    public void commit(Plan p, long[] timestampHlc, int[] expirySeconds) {
        LongBuffer ts = direct(8 * p.n).asLongBuffer();
        IntBuffer ex = direct(4 * p.n).asIntBuffer();
        ts.put(timestampHlc, 0, p.n);
        ex.put(expirySeconds, 0, p.n);
        NativeRetainPlan.retainPlanCommit(engine, p.tenants, p.tenantOff, p.nTenants, p.opTenant, p.topics, p.topicOff, p.n, p.action, ts, ex, p.info[0], p.info[1],
            null);
    }
}
