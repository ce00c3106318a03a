/*
 * EnginePackedColumns -- a decoded batch of logs as typed columns whose five narrow columns are
 * bit-packed (clg_packed, include/clonos_engine.h; the format: clonos_amd/csrc/pack.h): what
 * crossed the link is the bits the values hold, not a byte per tag and eight per timestamp.
 *
 * LogReplayerImpl pops one typed value at a time (LogReplayerImpl.java:61-119), so nothing is
 * unpacked into arrays here: a Cursor walks one span's blocks in place.
 *
 *   Cursor.nextTag()        the next determinant's tag        (LogReplayerImpl.java:61-119: each
 *                                                              replay* call checks it first)
 *   Cursor.nextChannel()    a byte  <- stream ORDER           (replayNextChannel, :71-78)
 *   Cursor.nextTimestamp()  a long  <- stream TIMESTAMP       (replayNextTimestamp, :81-88)
 *   Cursor.nextInt()        an int  <- stream RNG             (replayRandomInt, :61-68)
 *   Cursor.nextBufferSize() an int  <- stream BUFFER_BUILT    (SubpartitionRecoveryThread,
 *                                                              ReplayingState.java:161-188)
 *
 * A stream of n values is ceil(n / 1024) blocks; block b of stream c is descriptor
 * blkBase[c] + b: {ref i64, first i64, pos u64, width u32, count u32}, 32 bytes.  Value i of a
 * FOR block (tags, channels, ints) is ref + p_i; of a DELTA block (timestamps) it is first for
 * i = 0 and the previous value + ref + p_{i-1} after that, modulo 2^64.  p_j is the width-bit
 * little-endian field at bit j * width of the payload at bits[pos ...].  The wide rows, spanBase
 * and the payload column are EngineDecodedColumns' (classes ORDER, TIMESTAMP, RNG, BUFFER_BUILT,
 * WIDE).
 *
 * Source-only: this container has no JDK, so the binding is not compiled here.
 */
package org.apache.flink.runtime.causal.engine;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

public final class EnginePackedColumns {

	public static final int TAG = 0, ORDER = 1, TIMESTAMP = 2, RNG = 3, BUFFER_BUILT = 4, STREAMS = 5;
	public static final int BLOCK = 1024, DESC_BYTES = 32;
	static final int CLASSES = 5, WIDE = 4;

	final ByteBuffer desc, bits;
	final ByteBuffer wIdx, wRc, wV1, wVarOff, wVarLen, wSub, wV0;
	ByteBuffer var, varPos;
	final long[] spanBase;
	final long[] nVal = new long[STREAMS];
	final long[] blkBase = new long[STREAMS + 1];
	private final int nSpans;
	private long nRec;
	long nBits;
	private int errStatus, errSpan, errTag;
	private long errOff;

	/** Direct buffers of exactly the sizes a sizes-only call reported (result as nDecodeLogsColumnsPacked's). */
	EnginePackedColumns(long[] sizes, int nSpans, boolean withPayloads) {
		this.nSpans = nSpans;
		this.spanBase = new long[CLASSES * (nSpans + 1)];
		this.desc = direct(DESC_BYTES * sizes[23]);
		this.bits = direct(sizes[24]);
		final long w = sizes[5];
		this.wIdx = direct(4 * w);
		this.wRc = direct(4 * w);
		this.wV1 = direct(8 * w);
		this.wVarOff = direct(4 * w);
		this.wVarLen = direct(4 * w);
		this.wSub = direct(w);
		this.wV0 = direct(8 * w);
		if (withPayloads) {
			this.var = direct(sizes[11]);
			this.varPos = direct(8 * (sizes[10] + 1));
		}
		setResult(sizes);
	}

	private static ByteBuffer direct(long bytes) {
		return ByteBuffer.allocateDirect((int) Math.max(1, bytes)).order(ByteOrder.nativeOrder());
	}

	void setResult(long[] res) {
		this.nRec = res[0];
		this.errStatus = (int) res[6];
		this.errSpan = (int) res[7];
		this.errOff = res[8];
		this.errTag = (int) res[9];
		System.arraycopy(res, 13, nVal, 0, STREAMS);
		System.arraycopy(res, 18, blkBase, 0, STREAMS + 1);
		this.nBits = res[24];
	}

	public int spans() {
		return nSpans;
	}

	public long records() {
		return nRec;
	}

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

	/** The delivered size in bytes: descriptors, payload bits, wide rows, span bases, payload column. */
	public long deliveredBytes() {
		long n = DESC_BYTES * blkBase[STREAMS] + bits.capacity() + 33L * wSub.capacity() + 8L * spanBase.length;
		return var != null ? n + var.capacity() + varPos.capacity() : n;
	}

	/** Class-c records before span s (s == spans(): the totals). */
	public long base(int s, int c) {
		return spanBase[CLASSES * s + c];
	}

	public boolean hasPayloads() {
		return var != null;
	}

	/** Wide row k's payload: a slice of the payload column, not a copy. */
	public ByteBuffer payload(int k) {
		if (var == null) {
			throw new IllegalStateException("decoded without payloads");
		}
		final ByteBuffer d = var.duplicate();
		d.position((int) varPos.getLong(8 * k));
		d.limit((int) varPos.getLong(8 * (k + 1)));
		return d.slice();
	}

	/** A cursor over span s: LogReplayerImpl's determinant stream, one typed value at a time. */
	public Cursor cursor(int s) {
		return new Cursor(s);
	}

	/** One stream's position: the current block's descriptor, and for timestamps the running value. */
	private final class Stream {
		final int stream;
		long next, end;      // value indices in the stream
		long ref, pos, acc;   // the current block's reference and payload offset; the last timestamp
		int width;            // ... and its width
		long blockFirst = -1; // the stream index of the current block's first value (-1: none loaded)

		Stream(int stream, long first, long end) {
			this.stream = stream;
			this.next = first;
			this.end = end;
		}

		/** Residual j of the current block: the width-bit field at bit j * width of its payload. */
		private long field(long j) {
			if (width == 0) {
				return 0;
			}
			final long bit = j * width;
			final int at = (int) (pos + (bit >>> 6) * 8), sh = (int) (bit & 63);
			long v = bits.getLong(at) >>> sh;
			if (sh + width > 64) {
				v |= bits.getLong(at + 8) << (64 - sh);
			}
			return width == 64 ? v : v & ((1L << width) - 1);
		}

		private void load(long block) {
			final int d = (int) ((blkBase[stream] + block) * DESC_BYTES);
			ref = desc.getLong(d);
			acc = desc.getLong(d + 8);
			pos = desc.getLong(d + 16);
			width = desc.getInt(d + 24);
			blockFirst = block * BLOCK;
		}

		long next() {
			if (next >= end) {
				throw new IllegalStateException("stream " + stream + " is finished");
			}
			final long i = next++;
			final long block = i / BLOCK, k = i % BLOCK;
			if (stream != TIMESTAMP) {
				if (blockFirst != block * BLOCK) {
					load(block);
				}
				return ref + field(k);
			}
			if (blockFirst != block * BLOCK) { // a span may begin inside a block: run up to its first value
				load(block);
				for (long j = 1; j <= k; j++) {
					acc += ref + field(j - 1);
				}
				return acc;
			}
			acc += ref + field(k - 1);
			return acc;
		}
	}

	public final class Cursor {
		private final Stream[] st = new Stream[STREAMS];
		private int peeked = -1;

		Cursor(int s) {
			long r0 = 0, r1 = 0;
			for (int c = 0; c < CLASSES; c++) {
				r0 += base(s, c);
				r1 += base(s + 1, c);
			}
			st[TAG] = new Stream(TAG, r0, r1);
			for (int c = 0; c < 4; c++) {
				st[c + 1] = new Stream(c + 1, base(s, c), base(s + 1, c));
			}
		}

		public boolean isFinished() {
			return peeked < 0 && st[TAG].next >= st[TAG].end;
		}

		/** The next determinant's tag (Determinant.java:23-34), consumed: every replay* call of
		 *  LogReplayerImpl (LogReplayerImpl.java:61-119) checks it before it reads the value. */
		public int nextTag() {
			if (peeked >= 0) {
				final int t = peeked;
				peeked = -1;
				return t;
			}
			return (int) st[TAG].next();
		}

		/** The next tag without consuming it. */
		public int peekTag() {
			if (peeked < 0) {
				peeked = (int) st[TAG].next();
			}
			return peeked;
		}

		/** replayNextChannel (LogReplayerImpl.java:71-78): OrderDeterminant.getChannel, a Java byte. */
		public byte nextChannel() {
			return (byte) st[ORDER].next();
		}

		/** replayNextTimestamp (LogReplayerImpl.java:81-88): TimestampDeterminant.getTimestamp. */
		public long nextTimestamp() {
			return st[TIMESTAMP].next();
		}

		/** replayRandomInt (LogReplayerImpl.java:61-68): RNGDeterminant.getNumber. */
		public int nextInt() {
			return (int) st[RNG].next();
		}

		/** SubpartitionRecoveryThread.run (ReplayingState.java:161-188): BufferBuiltDeterminant's size. */
		public int nextBufferSize() {
			return (int) st[BUFFER_BUILT].next();
		}
	}
}
