/*
 * EngineDecodedColumns -- a decoded batch of logs as typed columns (clg_columns,
 * include/clonos_engine.h): what LogReplayerImpl (LogReplayerImpl.java:61-119) consumes one
 * typed value at a time, without the 13-byte rows around it.
 *
 *   replayNextChannel()   a byte   <- order        (OrderDeterminant.getChannel)
 *   replayNextTimestamp() a long   <- timestamp    (TimestampDeterminant.getTimestamp)
 *   replayRandomInt()     an int   <- rng          (RNGDeterminant.getNumber)
 *   SubpartitionRecoveryThread (ReplayingState.java:161-188) int sizes <- bufferBuilt
 *
 * Each column holds its class's values in record order over all spans (one span per log);
 * tag is the decode's tag stream, the interleaving; the w* buffers are the side rows of the
 * wide determinants (TimerTrigger, SourceCheckpoint, IgnoreCheckpoint, Serializable) with their
 * first field in wV0.  spanBase[5 s + c] counts the class-c records before span s (classes:
 * ORDER, TIMESTAMP, RNG, BUFFER_BUILT, WIDE), so the per-span views below are slices, not copies.
 * Record byte offsets are not part of the columns: EngineDecodedLog keeps those.
 *
 * Source-only: this container has no JDK, so the binding is not compiled here.
 */
package org.apache.flink.runtime.causal.engine;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.IntBuffer;
import java.nio.LongBuffer;

public final class EngineDecodedColumns {

	public static final int ORDER = 0, TIMESTAMP = 1, RNG = 2, BUFFER_BUILT = 3, WIDE = 4, CLASSES = 5;

	final ByteBuffer tag, order, timestamp, rng, bufferBuilt;
	final ByteBuffer wIdx, wRc, wV1, wVarOff, wVarLen, wSub, wV0;
	/** The payload column (decodeLogsColumns(..., true)), else null: the wide rows' payload bytes packed in
	 *  row order, and nWide + 1 longs, row k's bytes at var[varPos[k], varPos[k + 1]). */
	ByteBuffer var, varPos;
	final long[] spanBase;
	private final int nSpans;
	private long nRec;
	private int errStatus, errSpan, errTag;
	private long errOff;

	/** Direct buffers of exactly the sizes a sizes-only call reported (result as nDecodeLogsColumns'). */
	EngineDecodedColumns(long[] sizes, int nSpans) {
		this.nSpans = nSpans;
		this.spanBase = new long[CLASSES * (nSpans + 1)];
		this.tag = direct(sizes[0]);
		this.order = direct(sizes[1]);
		this.timestamp = direct(8 * sizes[2]);
		this.rng = direct(4 * sizes[3]);
		this.bufferBuilt = direct(4 * sizes[4]);
		final long w = sizes[5];
		this.wIdx = direct(4 * w);
		this.wRc = direct(4 * w);
		this.wV1 = direct(8 * w);
		this.wVarOff = direct(4 * w);
		this.wVarLen = direct(4 * w);
		this.wSub = direct(w);
		this.wV0 = direct(8 * w);
		setResult(sizes);
	}

	private static ByteBuffer direct(long bytes) {
		return ByteBuffer.allocateDirect((int) Math.max(1, bytes)).order(ByteOrder.nativeOrder());
	}

	void allocatePayloads(long nRows, long nVar) {
		this.var = direct(nVar);
		this.varPos = direct(8 * (nRows + 1));
	}

	public boolean hasPayloads() {
		return var != null;
	}

	/** Wide row k's payload (a TimerTrigger's name, a SourceCheckpoint's storage reference, a Serializable
	 *  record's java stream; empty for a row without one): a slice of the payload column, not a copy.  k counts
	 *  the batch's wide rows; span s's first is base(s, WIDE). */
	public ByteBuffer payload(int k) {
		if (var == null) {
			throw new IllegalStateException("decoded without payloads");
		}
		final long a = varPos.getLong(8 * k), b = varPos.getLong(8 * (k + 1));
		return slice(var, a, b - a, 1);
	}

	void setResult(long[] res) {
		this.nRec = res[0];
		this.errStatus = (int) res[6];
		this.errSpan = (int) res[7];
		this.errOff = res[8];
		this.errTag = (int) res[9];
	}

	public int spans() {
		return nSpans;
	}

	public long records() {
		return nRec;
	}

	/** The decode's first error (CLG_OK: none): span, span-relative offset and tag of the failing record.
	 *  The columns hold each span's records up to its first error. */
	public int errStatus() {
		return errStatus;
	}

	public int errSpan() {
		return errSpan;
	}

	public long errOff() {
		return errOff;
	}

	public int errTag() {
		return errTag;
	}

	/** Class-c records before span s (s == spans(): the totals). */
	public long base(int s, int c) {
		return spanBase[CLASSES * s + c];
	}

	public long count(int s, int c) {
		return base(s + 1, c) - base(s, c);
	}

	private static ByteBuffer slice(ByteBuffer b, long first, long n, int width) {
		final ByteBuffer d = b.duplicate().order(ByteOrder.nativeOrder());
		d.position((int) (first * width));
		d.limit((int) ((first + n) * width));
		return d.slice().order(ByteOrder.nativeOrder());
	}

	/** Span s's tag stream: one byte per record, in record order. */
	public ByteBuffer tags(int s) {
		long first = 0, n = 0;
		for (int c = 0; c < CLASSES; c++) {
			first += base(s, c);
			n += count(s, c);
		}
		return slice(tag, first, n, 1);
	}

	/** Span s's input channels (replayNextChannel's values), in record order. */
	public ByteBuffer channels(int s) {
		return slice(order, base(s, ORDER), count(s, ORDER), 1);
	}

	/** Span s's timestamps (replayNextTimestamp's values). */
	public LongBuffer timestamps(int s) {
		return slice(timestamp, base(s, TIMESTAMP), count(s, TIMESTAMP), 8).asLongBuffer();
	}

	/** Span s's random numbers (replayRandomInt's values). */
	public IntBuffer randomInts(int s) {
		return slice(rng, base(s, RNG), count(s, RNG), 4).asIntBuffer();
	}

	/** Span s's BufferBuilt sizes (SubpartitionRecoveryThread's). */
	public IntBuffer bufferSizes(int s) {
		return slice(bufferBuilt, base(s, BUFFER_BUILT), count(s, BUFFER_BUILT), 4).asIntBuffer();
	}

	/** Span s's wide rows: their record counts (AsyncDeterminant.getRecordCount) and first fields. */
	public IntBuffer wideRecordCounts(int s) {
		return slice(wRc, base(s, WIDE), count(s, WIDE), 4).asIntBuffer();
	}

	public LongBuffer wideValues(int s) {
		return slice(wV0, base(s, WIDE), count(s, WIDE), 8).asLongBuffer();
	}

	public LongBuffer wideSecondValues(int s) {
		return slice(wV1, base(s, WIDE), count(s, WIDE), 8).asLongBuffer();
	}

	/** Span-relative offset and length of a wide row's name, storage reference or java stream. */
	public IntBuffer wideVarOffsets(int s) {
		return slice(wVarOff, base(s, WIDE), count(s, WIDE), 4).asIntBuffer();
	}

	public IntBuffer wideVarLengths(int s) {
		return slice(wVarLen, base(s, WIDE), count(s, WIDE), 4).asIntBuffer();
	}

	public ByteBuffer wideSubs(int s) {
		return slice(wSub, base(s, WIDE), count(s, WIDE), 1);
	}
}
