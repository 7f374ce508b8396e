/*
 * The dist worker's fan-out split hinter (bifromq-dist/bifromq-dist-worker/src/main/java/org/apache/bifromq/dist/worker/hinter/FanoutSplitHinter.java)
 * without the RocksDB reader: the two questions doEstimate asks per key prefix of a mutation batch (:174-204) go to the engine, which holds the
 * range's route keys in device memory --
 *   how many records lie under the prefix:          ONE NativeHinter.routesPrefixCensus call for every prefix of the batch (:175-178),
 *   which key lies splitAtScale steps behind it:     NativeGc.routesWindow, chained behind the last key of the window before when
 *                                                    splitAtScale exceeds one window of 65 536 keys (:187-198; the default scale is 100 000).
 * The prefix of a mutated route is its FILTER's (tenantRouteStartKey: all receivers of the filter, normal and shared, lie under it), which is
 * what the names matchRecordKeyPrefix and fanout_topicfilters intend; bifromq_amd/hinter.py is the same state machine and is what the tests
 * run.  Deviation: the scale is the exact count of live keys under the prefix after the batch, not size / avgRecordSize minus tombstones.
 * recordMutate must run AFTER the batch was applied to the engine.  NOT compiled in this repository (no JDK in its build image).
 */
package org.apache.bifromq.routes.gpu;

import com.google.protobuf.ByteString;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.IntBuffer;
import java.nio.LongBuffer;
import java.util.ArrayList;
import java.util.List;
import java.util.Map;
import java.util.TreeMap;
import java.util.TreeSet;
import org.apache.bifromq.basekv.proto.Boundary;
import org.apache.bifromq.basekv.proto.SplitHint;
import org.apache.bifromq.basekv.store.proto.ROCoProcInput;
import org.apache.bifromq.basekv.store.proto.RWCoProcInput;
import org.apache.bifromq.basekv.store.range.hinter.IKVLoadRecord;
import org.apache.bifromq.basekv.store.range.hinter.IKVRangeSplitHinter;
import org.apache.bifromq.basekv.utils.BoundaryUtil;
import org.apache.bifromq.dist.rpc.proto.DistServiceRWCoProcInput;
import org.apache.bifromq.dist.rpc.proto.MatchRoute;
import org.apache.bifromq.dist.worker.schema.KVSchemaUtil;

public final class GpuFanoutSplitHinter implements IKVRangeSplitHinter {
    public static final String TYPE = "fanout_split_hinter";
    private static final int WINDOW_MAX = 65536; // BMQ_WINDOW_MAX

    private static final class Split {
        final long dataSize;
        final long recordSize;
        final ByteString splitKey;

        Split(long dataSize, long recordSize, ByteString splitKey) {
            this.dataSize = dataSize;
            this.recordSize = recordSize;
            this.splitKey = splitKey;
        }
    }

    private final long engine;
    private final int splitAtScale;
    // prefix -> split, in byte order of the prefixes: estimate() reports the smallest
    private final TreeMap<ByteString, Split> splits = new TreeMap<>(ByteString.unsignedLexicographicalComparator());
    private Boundary boundary;

    public GpuFanoutSplitHinter(long engine, int splitAtScale, Boundary boundary) {
        this.engine = engine;
        this.splitAtScale = splitAtScale;
        this.boundary = boundary;
    }

    private static ByteBuffer direct(int bytes) {
        return ByteBuffer.allocateDirect(Math.max(bytes, 1)).order(ByteOrder.nativeOrder());
    }

    @Override
    public void recordQuery(ROCoProcInput input, IKVLoadRecord ioRecord) {
    }

    @Override
    public synchronized void recordMutate(RWCoProcInput input, IKVLoadRecord ioRecord) {
        DistServiceRWCoProcInput dist = input.getDistService();
        TreeSet<ByteString> touched = new TreeSet<>(ByteString.unsignedLexicographicalComparator());
        switch (dist.getTypeCase()) {
            case BATCHMATCH ->
                dist.getBatchMatch().getRequestsMap().forEach((tenantId, records) -> collect(tenantId, records.getRouteList(), touched));
            case BATCHUNMATCH ->
                dist.getBatchUnmatch().getRequestsMap().forEach((tenantId, records) -> collect(tenantId, records.getRouteList(), touched));
            default -> {
            }
        }
        estimate(new ArrayList<>(touched));
    }

    private static void collect(String tenantId, List<MatchRoute> routes, TreeSet<ByteString> touched) {
        for (MatchRoute route : routes) {
            touched.add(KVSchemaUtil.tenantRouteStartKey(tenantId, route.getMatcher().getFilterLevelList()));
        }
    }

    @Override
    public synchronized void reset(Boundary boundary) {
        this.boundary = boundary;
        List<ByteString> again = new ArrayList<>();
        splits.entrySet().removeIf(e -> {
            boolean outside = !BoundaryUtil.inRange(e.getValue().splitKey, boundary);
            if (outside) {
                again.add(e.getKey());
            }
            return outside;
        });
        estimate(again);
    }

    @Override
    public synchronized SplitHint estimate() {
        SplitHint.Builder hint = SplitHint.newBuilder().setType(TYPE).putLoad("fanout_topicfilters", splits.size()).putLoad("fanout_scale", 0);
        Map.Entry<ByteString, Split> first = splits.firstEntry();
        if (first != null) {
            Split s = first.getValue();
            if (BoundaryUtil.isSplittable(boundary, s.splitKey)) {
                hint.setSplitKey(s.splitKey).putLoad("fanout_scale", s.dataSize / (double) s.recordSize);
            } else {
                splits.remove(first.getKey());
            }
        }
        return hint.build();
    }

    @Override
    public void close() {
    }

    // one census for all prefixes (in calls of PREFIX_MAX), then a split key for every candidate that has none yet
    private void estimate(List<ByteString> prefixes) {
        for (int at = 0; at < prefixes.size(); at += NativeHinter.PREFIX_MAX) {
            List<ByteString> part = prefixes.subList(at, Math.min(prefixes.size(), at + NativeHinter.PREFIX_MAX));
            int bytes = 0;
            for (ByteString p : part) {
                bytes += p.size();
            }
            ByteBuffer packed = direct(bytes);
            IntBuffer off = direct(4 * (part.size() + 1)).asIntBuffer();
            off.put(0, 0);
            for (int i = 0; i < part.size(); i++) {
                part.get(i).copyTo(packed);
                off.put(i + 1, packed.position());
            }
            LongBuffer stats = direct(32 * part.size()).asLongBuffer();
            NativeHinter.routesPrefixCensus(engine, packed, off, part.size(), stats);
            for (int i = 0; i < part.size(); i++) {
                ByteString prefix = part.get(i);
                long scale = stats.get(4 * i) + stats.get(4 * i + 1) + stats.get(4 * i + 2);
                long dataSize = stats.get(4 * i + 3);
                if (scale >= splitAtScale) {
                    if (!splits.containsKey(prefix)) { // an entry keeps the key it has
                        ByteString key = keyAt(prefix, splitAtScale);
                        if (key != null) {
                            splits.put(prefix, new Split(dataSize, dataSize / scale, key));
                        }
                    }
                } else if (2 * scale < splitAtScale) {
                    splits.remove(prefix);
                }
            }
        }
    }

    // the key at `index` among the live keys >= prefix (not bounded by the prefix), null if there are not that many
    private ByteString keyAt(ByteString prefix, int index) {
        long left = (long) index + 1;
        ByteString cursor = prefix;
        boolean exclusive = false;
        IntBuffer ids = direct(4 * (int) Math.min(left, WINDOW_MAX)).asIntBuffer();
        while (true) {
            int want = (int) Math.min(left, WINDOW_MAX);
            ByteBuffer lo = direct(cursor.size());
            cursor.copyTo(lo);
            int got = NativeGc.routesWindow(engine, lo, cursor.size(), exclusive, want, ids, null);
            if (got < want) {
                return null;
            }
            ByteBuffer key = direct(512);
            int len = NativeGc.routeKey(engine, ids.get(got - 1), key);
            if (len < 0) { // -(the length needed)
                key = direct(-len);
                len = NativeGc.routeKey(engine, ids.get(got - 1), key);
            }
            key.limit(len);
            ByteString last = ByteString.copyFrom(key);
            left -= want;
            if (left == 0) {
                return last;
            }
            cursor = last;
            exclusive = true;
        }
    }
}
