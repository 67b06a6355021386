package org.apache.pinot.core.gpu;

import it.unimi.dsi.fastutil.doubles.DoubleArrayList;
import it.unimi.dsi.fastutil.doubles.DoubleOpenHashSet;
import it.unimi.dsi.fastutil.floats.FloatOpenHashSet;
import it.unimi.dsi.fastutil.ints.IntOpenHashSet;
import it.unimi.dsi.fastutil.longs.LongOpenHashSet;
import it.unimi.dsi.fastutil.objects.ObjectOpenHashSet;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.charset.StandardCharsets;
import java.util.List;
import org.apache.pinot.common.request.context.ExpressionContext;
import org.apache.pinot.common.utils.DataSchema;
import org.apache.pinot.common.utils.DataSchema.ColumnDataType;
import org.apache.pinot.core.query.aggregation.function.AggregationFunction;
import org.apache.pinot.core.query.request.context.QueryContext;
import org.apache.pinot.segment.spi.AggregationFunctionType;


/**
 * The DataSchema of a GPU group-by result, as GroupByOperator builds it (GroupByOperator.java:66-86): the group-by
 * expressions with the stored types of their key columns, then each function's result column name and intermediate
 * type.  Also the intermediate result of DISTINCTCOUNT: the value set the reference's convertToValueSet builds from its
 * dictId bitmap (BaseDistinctAggregateAggregationFunction.java:77-108), here from the result dictionary's values x the
 * row's bitset; and of PERCENTILE: the DoubleArrayList of matched values (PercentileAggregationFunction.java:77-94),
 * here each value of the result dictionary repeated by the row's histogram count, ascending (the reference sorts the list
 * before it reads an element, :146-158).  (Written against the reference API; not compiled in this repository's build.)
 */
final class GpuResultSchema {
  private GpuResultSchema() {
  }

  static ColumnDataType keyType(int phType) {
    switch (phType) {
      case PinotHipJni.INT: return ColumnDataType.INT;
      case PinotHipJni.LONG: return ColumnDataType.LONG;
      case PinotHipJni.FLOAT: return ColumnDataType.FLOAT;
      case PinotHipJni.DOUBLE: return ColumnDataType.DOUBLE;
      default: return ColumnDataType.STRING;
    }
  }

  /** An aggregation whose intermediate result is an object built from a per-row table over a result dictionary. */
  interface RowObjects {
    Object row(int row);
  }

  /** The object column of aggregation {@code k}, or null when its intermediate result is a plain value. */
  static RowObjects rowObjects(long res, int k, AggregationFunction f) {
    if (f.getType() == AggregationFunctionType.DISTINCTCOUNT) {
      return new DistinctColumn(res, k);
    }
    if (f.getType() == AggregationFunctionType.PERCENTILE) {
      return new HistogramColumn(res, k);
    }
    return null;
  }

  /** PERCENTILE aggregation {@code k} of a result (ph_result_percentile_*): uint32[D] histogram rows over the D values
   *  of its result dictionary. */
  static final class HistogramColumn implements RowObjects {
    private final int _type;
    private final int _entrySize;
    private final long _count;
    private final ByteBuffer _hist;
    private final ByteBuffer _values;

    HistogramColumn(long res, int k) {
      int[] te = new int[2];
      _count = PinotHipJni.resultPercentileDictionary(res, k, te);
      _type = te[0];
      _entrySize = te[1];
      _hist = PinotHipJni.resultAggregationBuffer(res, k, 4 * (int) Math.max(1, _count)).order(ByteOrder.nativeOrder());
      _values = PinotHipJni.resultPercentileValues(res, k).order(ByteOrder.nativeOrder());
    }

    /** Row {@code row}: the matched values as doubles (getDoubleValuesSV's conversion), ascending. */
    @Override
    public Object row(int row) {
      DoubleArrayList list = new DoubleArrayList();
      long stride = Math.max(1, _count);
      for (int i = 0; i < _count; i++) {
        long n = _hist.getInt((int) (4 * (row * stride + i))) & 0xffffffffL;
        if (n == 0) {
          continue;
        }
        double v;
        switch (_type) {
          case PinotHipJni.INT: v = _values.getInt(_entrySize * i); break;
          case PinotHipJni.LONG: v = (double) _values.getLong(_entrySize * i); break;
          case PinotHipJni.FLOAT: v = _values.getFloat(_entrySize * i); break;
          default: v = _values.getDouble(_entrySize * i);
        }
        for (long j = 0; j < n; j++) {
          list.add(v);
        }
      }
      return list;
    }
  }

  /** DISTINCTCOUNT aggregation {@code k} of a result: its dictionary and buffers are fetched once (three JNI calls, two
   *  direct buffers over the whole column), then {@link #set} builds any row's value set from them. */
  static final class DistinctColumn implements RowObjects {
    private final int _type;
    private final int _entrySize;
    private final int _words;
    private final long _count;
    private final ByteBuffer _bits;
    private final ByteBuffer _values;

    DistinctColumn(long res, int k) {
      int[] tew = new int[3];
      _count = PinotHipJni.resultDistinctDictionary(res, k, tew);
      _type = tew[0];
      _entrySize = tew[1];
      _words = tew[2];
      _bits = PinotHipJni.resultAggregationBuffer(res, k, 4 * _words).order(ByteOrder.nativeOrder());
      _values = PinotHipJni.resultDistinctValues(res, k).order(ByteOrder.nativeOrder());
    }

    @Override
    public Object row(int row) {
      return set(row);
    }

    /** Row {@code row}: IntOpenHashSet / LongOpenHashSet / FloatOpenHashSet / DoubleOpenHashSet /
     *  ObjectOpenHashSet<String> by the column's stored type. */
    Object set(int row) {
      IntOpenHashSet ints = _type == PinotHipJni.INT ? new IntOpenHashSet() : null;
      LongOpenHashSet longs = _type == PinotHipJni.LONG ? new LongOpenHashSet() : null;
      FloatOpenHashSet floats = _type == PinotHipJni.FLOAT ? new FloatOpenHashSet() : null;
      DoubleOpenHashSet doubles = _type == PinotHipJni.DOUBLE ? new DoubleOpenHashSet() : null;
      ObjectOpenHashSet<String> strings = _type == PinotHipJni.STRING ? new ObjectOpenHashSet<>() : null;
      int es = _entrySize;
      for (int word = 0; word < _words; word++) {
        int x = _bits.getInt(4 * (row * _words + word));
        while (x != 0) {
          int i = 32 * word + Integer.numberOfTrailingZeros(x);
          x &= x - 1;
          if (i >= _count) {
            break;
          }
          switch (_type) {
            case PinotHipJni.INT: ints.add(_values.getInt(es * i)); break;
            case PinotHipJni.LONG: longs.add(_values.getLong(es * i)); break;
            case PinotHipJni.FLOAT: floats.add(_values.getFloat(es * i)); break;
            case PinotHipJni.DOUBLE: doubles.add(_values.getDouble(es * i)); break;
            default: {
              byte[] b = new byte[es];
              for (int j = 0; j < es; j++) {
                b[j] = _values.get(es * i + j);
              }
              int len = 0;
              while (len < es && b[len] != 0) {
                len++;
              }
              strings.add(new String(b, 0, len, StandardCharsets.UTF_8));
            }
          }
        }
      }
      return ints != null ? ints : longs != null ? longs : floats != null ? floats : doubles != null ? doubles : strings;
    }
  }

  static DataSchema of(QueryContext ctx, long res) {
    List<ExpressionContext> groupBy = ctx.getGroupByExpressions();
    AggregationFunction[] functions = ctx.getAggregationFunctions();
    int nk = groupBy.size();
    String[] names = new String[nk + functions.length];
    ColumnDataType[] types = new ColumnDataType[nk + functions.length];
    for (int g = 0; g < nk; g++) {
      names[g] = groupBy.get(g).toString();
      types[g] = keyType(PinotHipJni.resultKeyType(res, g));
    }
    for (int k = 0; k < functions.length; k++) {
      // a filtered function's column carries its FilterContext (AggregationFunctionUtils.getResultColumnName :269-275),
      // the name ph_result_datatable writes too
      names[nk + k] = ctx.hasFilteredAggregations()
          ? org.apache.pinot.core.query.aggregation.function.AggregationFunctionUtils.getResultColumnName(functions[k],
              ctx.getFilteredAggregationFunctions().get(k).getRight())
          : functions[k].getResultColumnName();
      types[nk + k] = functions[k].getIntermediateResultColumnType();
    }
    return new DataSchema(names, types);
  }
}
